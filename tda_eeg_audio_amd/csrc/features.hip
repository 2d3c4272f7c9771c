// features.hip -- small per-window kernels around the Rips core, gfx950 / wave64.
//
//   tau_kernel        replaces compute_tau                  (scripts/utils.py:92-104)
//   features_kernel   replaces extract_features             (scripts/utils.py:144-177)
//                     == extract_persistence_features       (tda_eeg_classification_v2.py:179-250)
//   aggregate_kernel  replaces the mean/std over windows    (tda_eeg_classification_v2.py:429-436)
//   temporal_corr_kernel  replaces the window filter and the spearmanr loop, r and p   (tda_eeg_audio_comparison.py:90-91,104-114)
//
// All float64.  Sums follow numpy's pairwise-summation tree (8 interleaved partial sums for
// n <= 128, halving above) so that mean/std agree with np.mean/np.std to the last bit on the
// same input order; log() is OCML's, so the entropy is compared with a 1e-12 tolerance.
#include "common.h"
#include <climits>

// numpy's pairwise sum over f(lo) .. f(lo+n-1), evaluated redundantly by every lane that
// calls it (n is tiny: <= a few hundred).  The leaf (n <= 128: every diagram and group of the path) is inlined into
// its caller -- as a (recursive) call per sum the finishing pass of a step took 1.6x as long.
template <class F>
__device__ __forceinline__ double np_pairwise_leaf(const F& f, int lo, int n)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += f(lo + i);
        return res;
    }
    double r0 = f(lo), r1 = f(lo + 1), r2 = f(lo + 2), r3 = f(lo + 3);
    double r4 = f(lo + 4), r5 = f(lo + 5), r6 = f(lo + 6), r7 = f(lo + 7);
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += f(lo + i + 0); r1 += f(lo + i + 1); r2 += f(lo + i + 2); r3 += f(lo + i + 3);
        r4 += f(lo + i + 4); r5 += f(lo + i + 5); r6 += f(lo + i + 6); r7 += f(lo + i + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += f(lo + i);
    return res;
}
template <class F>
__device__ __forceinline__ double np_pairwise_split_uniform(const F& f, int lo_, int n_)        // n > 128 (off the usual path)
{
    // numpy halves recursively (left part a multiple of 8) down to leaves of <= 128: the same tree, walked with an
    // explicit stack.  UNIFORM flavour: every lane of the wave evaluates the same sum, so frame i of the stack lives in LANE i of four
    // registers (select / v_readlane with the wave-uniform stack pointer): no calls, no scratch memory.
    const int lo = uni(lo_), n = uni(n_);
    int vlo = 0, vn = 0, vph = 0, vl0 = 0, vl1 = 0;
    int sp = 0;
    const int me = lane_id();
    double ret = 0.0;
    vlo = me == 0 ? (lo) : vlo;
    vn = me == 0 ? (n) : vn;
    while (sp >= 0) {
        const int flo = __builtin_amdgcn_readlane(vlo, sp), fn = __builtin_amdgcn_readlane(vn, sp);
        const int ph = __builtin_amdgcn_readlane(vph, sp);
        if (fn <= 128) { ret = uni_f64(np_pairwise_leaf(f, flo, fn), 0); --sp; continue; }
        int n2 = fn / 2;
        n2 -= n2 % 8;
        if (ph == 0) {
            vph = me == sp ? (1) : vph;
            ++sp;
            vlo = me == sp ? (flo) : vlo; vn = me == sp ? (n2) : vn;
            vph = me == sp ? (0) : vph;
        } else if (ph == 1) {
            const long long bits = __double_as_longlong(ret);
            vl0 = me == sp ? ((int)(unsigned)(bits & 0xffffffffll)) : vl0;
            vl1 = me == sp ? ((int)(unsigned)((unsigned long long)bits >> 32)) : vl1;
            vph = me == sp ? (2) : vph;
            ++sp;
            vlo = me == sp ? (flo + n2) : vlo; vn = me == sp ? (fn - n2) : vn;
            vph = me == sp ? (0) : vph;
        } else {
            const unsigned l0 = (unsigned)__builtin_amdgcn_readlane(vl0, sp), l1 = (unsigned)__builtin_amdgcn_readlane(vl1, sp);
            ret = __longlong_as_double((long long)(((unsigned long long)l1 << 32) | l0)) + ret;
            --sp;
        }
    }
    return ret;
}
// any-lane flavour (sums and lengths may differ from lane to lane): frames in private arrays, a real call -- used by
// the small per-group kernels, whose groups have <= 128 members on the whole path
template <class F>
__device__ __noinline__ double np_pairwise_split(const F& f, int lo, int n)
{
    int slo[26], sn[26], sph[26];
    double sleft[26];
    int sp = 0;
    double ret = 0.0;
    slo[0] = lo; sn[0] = n; sph[0] = 0; sleft[0] = 0.0;
    while (sp >= 0) {
        const int flo = slo[sp], fn = sn[sp];
        if (fn <= 128) { ret = np_pairwise_leaf(f, flo, fn); --sp; continue; }
        int n2 = fn / 2;
        n2 -= n2 % 8;
        if (sph[sp] == 0) { sph[sp] = 1; ++sp; slo[sp] = flo; sn[sp] = n2; sph[sp] = 0; }
        else if (sph[sp] == 1) { sleft[sp] = ret; sph[sp] = 2; ++sp; slo[sp] = flo + n2; sn[sp] = fn - n2; sph[sp] = 0; }
        else { ret = sleft[sp] + ret; --sp; }
    }
    return ret;
}
template <class F>
__device__ __forceinline__ double np_pairwise_fn(const F& f, int lo, int n)
{
    return n <= 128 ? np_pairwise_leaf(f, lo, n) : np_pairwise_split(f, lo, n);
}

__device__ __forceinline__ double np_pairwise_sum(const double* a, int n, int stride)
{
    auto f = [=](int i) { return a[(size_t)i * stride]; };
    return np_pairwise_fn(f, 0, n);
}
// the same sum and length in every lane of the wave (diagram_finish_kernel)
__device__ __forceinline__ double np_pairwise_sum_uniform(const double* a, int n)
{
    auto f = [=](int i) { return a[i]; };
    return n <= 128 ? np_pairwise_leaf(f, 0, n) : np_pairwise_split_uniform(f, 0, n);
}

// ---------------------------------------------------------------------------------
// compute_tau: first lag k in [1, min(max_lag, len)) whose autocorrelation is <= 0.
// One wave per window; the lags are walked in chunks of 64, lane l owning lag k0 + l of the chunk that starts at k0
// (any max_lag: the loop ends with the first chunk that holds a lag with ac <= 0), each lag a
// sequential fma chain over t (the order oracle/tda_oracle.c::orc_compute_tau fixes).
// ---------------------------------------------------------------------------------
// seg_off != nullptr: workgroup g handles the FIRST window of group g (tda_eeg_audio_comparison.py:83: tau is
// computed once per recording-band, from its first selected window) and also writes the value to every
// window of the group in tau_win, the per-window array the Takens kernel takes.
__global__ void __launch_bounds__(64)
tau_kernel(const double* __restrict__ win, int n_win, int n_t, int max_lag, int* __restrict__ tau,
           const int* __restrict__ seg_off, int* __restrict__ tau_win)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* sc = reinterpret_cast<double*>(smem);
    const int g = blockIdx.x;
    if (g >= n_win) return;                          // n_win = number of groups in segment mode
    const int lane = lane_id();
    int w = g, w_end = g + 1;
    if (seg_off) {
        w = seg_off[g]; w_end = seg_off[g + 1];
        if (w_end <= w) { if (lane == 0) tau[g] = 0; return; }      // empty group
    }
    const double* s = win + (size_t)w * n_t;
    for (int t = lane; t < n_t; t += 64) sc[t] = s[t];
    __syncthreads();
    double sum = 0.0;
    for (int t = 0; t < n_t; ++t) sum += sc[t];     // every lane: same sequential sum
    const double m = sum / (double)n_t;
    __syncthreads();
    for (int t = lane; t < n_t; t += 64) sc[t] = sc[t] - m;
    __syncthreads();
    if (max_lag < 0) max_lag = n_t / 4;             // utils.py:94-95
    if (max_lag > n_t - 1) max_lag = n_t - 1;       // utils.py:96
    const int lim = max_lag < n_t ? max_lag : n_t;  // utils.py:101
    int found = 0;
    for (int k0 = 1; k0 < lim && !found; k0 += 64) {
        const int k = k0 + lane;
        double acc = 1.0;
        if (k < lim) {
            acc = 0.0;
            for (int t = 0; t + k < n_t; ++t) acc = fma(sc[t + k], sc[t], acc);
        }
        const u64 bal = __ballot(k < lim && acc <= 0.0);
        if (bal) found = k0 + __builtin_ctzll(bal);
    }
    if (!found) { found = max_lag / 10; if (found < 1) found = 1; }
    if (lane == 0) tau[g] = found;
    if (tau_win)
        for (int i = w + lane; i < w_end; i += 64) tau_win[i] = found;
}

// ---------------------------------------------------------------------------------
// Finishing pass over the diagrams of a batch, up to four diagram sets in ONE launch, one wave per diagram:
//   * order != 0: the rows of an H1 diagram go into ripser's order (descending birth; ties: descending death, then
//     emission order) -- the Rips kernels emit them in the order of the kills;
//   * feat != NULL: extract_features, 11 scalars per diagram, key order of utils.py:166-177.
// This is latency-bound scalar work (a few dependent float64 sums over <= a few hundred rows): it wants many
// independent waves and little LDS each, which is why it is NOT an epilogue of the Rips kernels (an 80 KB
// workgroup would sit on its CU for the duration; measured: 13 % slower end to end).
// ---------------------------------------------------------------------------------
struct DiagramSets {
    double* rows[4]; const int* cnt[4]; int cap[4]; int order[4]; double* feat[4];
    int n_sets;
};

// Waves of a workgroup never meet: each has its own diagram and its own LDS slice, and the LDS serves the accesses
// of ONE wave in program order -- a compiler fence is all the synchronisation there is.  (Four diagrams per
// workgroup because a launch of 3 x 106,200 one-wave workgroups is bound by the dispatcher, not by the work.)
#define FIN_WAVES 4
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// A launch takes the diagrams with k_lo < rows <= lds_cap: the first one has slices of 64 rows (8 KB per workgroup:
// eight workgroups = every wave slot of a CU), a second one, sized by the capacities of the buffers (H1: 256 rows,
// 32 KB per workgroup, five per CU), the larger diagrams -- its other waves leave after one load.
// diagram g of a set, by the wave that calls it; b: the wave's LDS slice.  (The set's fields come as values: a reference
// to the kernel's DiagramSets argument would make a private copy of it, indexed in scratch memory.)
__device__ __forceinline__ void finish_wave(double* rows_set, const int* cnt_set, int cap, int order, double* feat, int g,
                                            int lds_cap, int k_lo, double* b)
{
    double* d = b + lds_cap;                           // births | deaths | pers | tmp, lds_cap each
    double* p = d + lds_cap;
    double* tmp = p + lds_cap;
    const int lane = lane_id();
    int k = cnt_set[g];
    k = k < cap ? k : cap;
    if (k > lds_cap || k <= k_lo) return;              // (wave-uniform: another launch's diagram)
    double* rows = rows_set + (size_t)g * cap * 2;
    const bool reorder = order && k >= 2;
    if (!reorder && !feat) return;
    // rows -> LDS (p, tmp serve as staging while the rows are put in order)
    double* rb = reorder ? p : b;
    double* rd = reorder ? tmp : d;
    for (int i = lane; i < k; i += 64) { rb[i] = rows[2 * i]; rd[i] = rows[2 * i + 1]; }
    wave_sync();
    if (reorder) {
        for (int i = lane; i < k; i += 64) {
            const double bi = rb[i], di = rd[i];
            int pos = 0;
            for (int j = 0; j < k; ++j) {
                const double bj = rb[j], dj = rd[j];
                pos += ((bj > bi) || (bj == bi && (dj > di || (dj == di && j < i)))) ? 1 : 0;
            }
            b[pos] = bi; d[pos] = di;
            if (pos != i) { rows[2 * pos] = bi; rows[2 * pos + 1] = di; }
        }
        wave_sync();
    }
    if (!feat) return;
    // compact finite rows in place, preserving order (utils.py:146-147): row i moves to pos <= i, and every lane
    // has read its row before any lane of the same trip writes
    int m = 0, ness = 0;
    for (int i0 = 0; i0 < k; i0 += 64) {
        const int i = i0 + lane;
        double bi = 0.0, di = 0.0;
        bool fin = false, valid = i < k;
        if (valid) { bi = b[i]; di = d[i]; fin = isfinite(bi) && isfinite(di); }
        const u64 bal = __ballot(fin);
        const int pos = m + __popcll(bal & ((1ull << lane) - 1ull));
        wave_sync();
        if (fin) { b[pos] = bi; d[pos] = di; p[pos] = di - bi; }
        m += __popcll(bal);
        ness += __popcll(__ballot(valid && !fin));
    }
    wave_sync();
    double out[TDA_N_FEATURES];
#pragma unroll
    for (int i = 0; i < TDA_N_FEATURES; ++i) out[i] = 0.0;
    out[1] = (double)ness;
    if (m > 0) {
        out[0] = (double)m;
        const double* arr[3] = {b, d, p};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double mean = np_pairwise_sum_uniform(arr[q], m) / (double)m;
            out[2 + 2 * q] = mean;
            if (m > 1) {
                wave_sync();
                for (int i = lane; i < m; i += 64) { const double z = arr[q][i] - mean; tmp[i] = z * z; }
                wave_sync();
                out[3 + 2 * q] = sqrt(np_pairwise_sum_uniform(tmp, m) / (double)m);
            }
        }
        double mx = -INFINITY;
        for (int i = lane; i < m; i += 64) mx = p[i] > mx ? p[i] : mx;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(mx, off, 64); mx = o > mx ? o : mx; }
        out[8] = mx;
        const double tot = np_pairwise_sum_uniform(p, m);
        out[9] = tot;
        if (m > 1 && tot > 0.0) {
            wave_sync();
            // pn = pers/sum; keep pn > 0 in order (utils.py:161-163)
            int c = 0;
            for (int i0 = 0; i0 < m; i0 += 64) {
                const int i = i0 + lane;
                double pn = 0.0;
                if (i < m) pn = p[i] / tot;
                const bool pos = i < m && pn > 0.0;
                const u64 bal = __ballot(pos);
                const int at = c + __popcll(bal & ((1ull << lane) - 1ull));
                if (pos) tmp[at] = pn * log(pn + 1e-10);
                c += __popcll(bal);
            }
            wave_sync();
            out[10] = -np_pairwise_sum_uniform(tmp, c) / log((double)m + 1e-10);
        }
    }
    if (lane < TDA_N_FEATURES) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < TDA_N_FEATURES; ++i) v = (lane == i) ? out[i] : v;
        feat[(size_t)g * TDA_N_FEATURES + lane] = v;
    }
}

__global__ void __launch_bounds__(64 * FIN_WAVES, 8)
diagram_finish_kernel(DiagramSets S, int n_dgm, int lds_cap, int k_lo)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wv = uni((int)(threadIdx.x >> 6));
    double* b = reinterpret_cast<double*>(smem) + (size_t)wv * 4 * lds_cap;
    const long long gi = (long long)blockIdx.x * (blockDim.x >> 6) + wv;
    const int set = (int)(gi / n_dgm), g = (int)(gi - (long long)set * n_dgm);
    if (set >= S.n_sets) return;
    finish_wave(S.rows[set], S.cnt[set], S.cap[set], S.order[set], S.feat[set], g, lds_cap, k_lo, b);
}

// The same for the diagrams on a list (those the packed kernel below leaves: more than FINP_ROWS rows), on a grid that
// does not depend on the batch: wave w of the grid takes entries w, w + waves, ...  [0] = entries, [1] = waves done (the
// last one through clears both, so the next packed launch appends from zero without a memset node in between:
// RETRY_SCAN_END of rips.hip), global diagram indices set * n_dgm + g from [4] on.
__global__ void __launch_bounds__(64 * FIN_WAVES)        // (its LDS allows five waves per SIMD: no need to squeeze into 64 VGPRs)
diagram_finish_list_kernel(DiagramSets S, int n_dgm, int lds_cap, int k_lo, int* list)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wv = uni((int)(threadIdx.x >> 6)), nw = (int)(blockDim.x >> 6);
    double* b = reinterpret_cast<double*>(smem) + (size_t)wv * 4 * lds_cap;
    const int n_all = S.n_sets * n_dgm;                // (the host checked that it fits an int)
    int nl = uni(list[0]);
    nl = nl < n_all ? nl : n_all;
    for (int j = (int)blockIdx.x * nw + wv; j < nl; j += (int)gridDim.x * nw) {
        const int gi = uni(list[4 + j]);
        if (gi >= 0 && gi < n_all) {
            const int set = gi / n_dgm;
            finish_wave(S.rows[set], S.cnt[set], S.cap[set], S.order[set], S.feat[set], gi - set * n_dgm, lds_cap, k_lo, b);
        }
        wave_sync();
    }
    if (lane_id() == 0 && atomicAdd(&list[1], 1) == (int)gridDim.x * nw - 1) { list[0] = 0; list[1] = 0; }
}

// ---------------------------------------------------------------------------------
// The packed finishing kernel: diagrams of at most FINP_ROWS = 64 rows (every diagram of the usual path: 12 to 47 rows),
// EIGHT lanes per diagram, so a wave finishes eight consecutive diagrams of one set (order, feat and cap are
// wave-uniform; the groups of a wave loop to the largest row count among them).  diagram_finish_kernel gives every sum
// of a diagram to all 64 lanes of its wave -- the same serial chain of m loads and m additions 64 times over, eight sums
// per diagram.  numpy's leaf IS eight independent accumulators, so here lane j of a group carries r_j (the same
// additions in the same order), the three combining steps ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) run on the DPP network
// inside the group (IEEE addition is commutative: which lane of a pair adds is free) and the n % 8 tail is added in order
// to the combined value: bit for bit np_pairwise_leaf.  Control flow diverges between groups only (a group's eight
// lanes take every branch together), and every DPP source lies in the reader's own group.
// LDS: births | deaths of a diagram, 1 KB; pers = d - b, (x - mean)^2 and pn * log(pn + 1e-10) come from the functor of
// the sum (the entropy terms are compacted over the births, which nobody reads any more by then).  Slices are
// FINP_STRIDE = 136 doubles apart: the 16 banks of skew put the eight-row reads of the four groups of a half-wave on
// 4 x 16 different banks (at 128 doubles all groups would meet on the same 16: a four-way conflict on every read).
// 8.5 KB per wave = 18 waves = 144 diagrams in flight per CU (diagram_finish_kernel: 32); the b | d | pers | tmp layout
// of diagram_finish_kernel would be 17 KB per wave and 9 waves per CU.  Chosen by this arithmetic, not by a measurement
// of both layouts.
// Rows are put in order by counting as before: lane j ranks rows j, j + 8, ... against all k rows of the slice, keeps
// the ranks as bytes of one 64-bit word, writes the rows to their places in HBM at once and moves births, then deaths
// inside the slice (eight values in registers between the reads and the writes).
// The maximum is the one value that is not computed in diagram_finish_kernel's order: it is order-free except for the
// sign of a zero maximum of a diagram that holds both +0 and -0 persistences (a death of -0: no Rips kernel emits one).
// A diagram with more than FINP_ROWS rows is appended to `list` (wave-aggregated, as retry_collect_kernel) for
// diagram_finish_list_kernel; list == NULL: no set has room for one.
// ---------------------------------------------------------------------------------
#define FINP_ROWS 64
#define FINP_STRIDE (2 * FINP_ROWS + 8)
#define FINP_WAVES 2

template <class F>
__device__ __forceinline__ double np_pairwise_group8(const F& f, int n, int sub)      // n <= 128, uniform in the group
{
    const int n8 = n & ~7;                             // n < 8: the serial loop alone (the "tail" from 0)
    double r = 0.0;
    if (n8) {
        r = f(sub);
        for (int i = 8; i < n8; i += 8) r += f(i + sub);
    }
    r += dpp_f64<0xB1, 0xF>(r);                        // quad_perm [1,0,3,2]: r0+r1, r2+r3, r4+r5, r6+r7
    r += dpp_f64<0x4E, 0xF>(r);                        // quad_perm [2,3,0,1]: (r0+r1)+(r2+r3), (r4+r5)+(r6+r7)
    r += dpp_f64<0x141, 0xF>(r);                       // row_half_mirror: lane j <-> 7 - j, the other quad's sum
    double res = n8 ? r : 0.0;
    for (int i = n8; i < n; ++i) res += f(i);
    return res;
}
// np.mean and np.std of f(0) .. f(m-1)
template <class F>
__device__ __forceinline__ void group8_mean_std(const F& f, int m, int sub, double& mean, double& sd)
{
    mean = np_pairwise_group8(f, m, sub) / (double)m;
    sd = 0.0;
    if (m > 1) {
        const double mu = mean;
        auto sq = [=](int i) { const double z = f(i) - mu; return z * z; };
        sd = sqrt(np_pairwise_group8(sq, m, sub) / (double)m);
    }
}

__global__ void __launch_bounds__(64 * FINP_WAVES)
diagram_finish_packed_kernel(DiagramSets S, int n_dgm, int* list)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wv = uni((int)(threadIdx.x >> 6));
    const int lane = lane_id(), grp = lane >> 3, sub = lane & 7;
    const int wps = (n_dgm + 7) >> 3;                  // waves per set: the last one of a set may have idle groups
    const long long wi = (long long)blockIdx.x * FINP_WAVES + wv;
    const int set = (int)(wi / wps);
    if (set >= S.n_sets) return;
    const int g = ((int)(wi - (long long)set * wps) << 3) + grp;
    const int cap = S.cap[set];
    const bool in = g < n_dgm;
    int k = 0;
    if (in) { k = S.cnt[set][g]; k = k < cap ? k : cap; }
    const bool big = in && k > FINP_ROWS;
    if (list) {
        const u64 bal = __ballot(big && sub == 0);
        if (bal) {
            const int lead = __builtin_ctzll(bal);
            int base = 0;
            if (lane == lead) base = atomicAdd(&list[0], __builtin_popcountll(bal));
            base = __builtin_amdgcn_readlane(base, lead);
            if (big && sub == 0) list[4 + base + __builtin_popcountll(bal & ((1ull << lane) - 1ull))] = set * n_dgm + g;
        }
    }
    double* feat = S.feat[set];
    const bool reorder = S.order[set] && k >= 2;
    if (!in || big || (!reorder && !feat)) return;     // (uniform in the group, as every branch below)
    double* b = reinterpret_cast<double*>(smem) + (size_t)(wv * 8 + grp) * FINP_STRIDE;
    double* d = b + FINP_ROWS;
    double* rows = S.rows[set] + (size_t)g * cap * 2;
    for (int i = sub; i < k; i += 8) { b[i] = rows[2 * i]; d[i] = rows[2 * i + 1]; }
    wave_sync();
    if (reorder) {
        u64 rank = 0;                                  // byte t: the place of row sub + 8 t
        for (int t = 0, i = sub; i < k; ++t, i += 8) {
            const double bi = b[i], di = d[i];
            int pos = 0;
            for (int j = 0; j < k; ++j) {
                const double bj = b[j], dj = d[j];
                pos += ((bj > bi) || (bj == bi && (dj > di || (dj == di && j < i)))) ? 1 : 0;
            }
            rank |= (u64)pos << (8 * t);
            if (pos != i) { rows[2 * pos] = bi; rows[2 * pos + 1] = di; }
        }
        if (!feat) return;
        for (int q = 0; q < 2; ++q) {
            double* a = q ? d : b;
            double v[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = sub + 8 * t < k ? a[sub + 8 * t] : 0.0;
            wave_sync();
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (sub + 8 * t < k) a[(int)(rank >> (8 * t)) & 63] = v[t];
            wave_sync();
        }
    }
    if (!feat) return;
    // compact finite rows in place, preserving order (utils.py:146-147), eight rows per trip: row i moves to pos <= i, and
    // every lane has read its row before any lane of the same trip writes.  A group's byte of the ballot is its own.
    int m = 0;
    for (int i0 = 0; i0 < k; i0 += 8) {
        const int i = i0 + sub;
        double bi = 0.0, di = 0.0;
        bool fin = false;
        if (i < k) { bi = b[i]; di = d[i]; fin = isfinite(bi) && isfinite(di); }
        const u32 bal = (u32)(__ballot(fin) >> (8 * grp)) & 0xffu;
        const int pos = m + __popc(bal & ((1u << sub) - 1u));
        wave_sync();
        if (fin) { b[pos] = bi; d[pos] = di; }
        m += __popc(bal);
    }
    wave_sync();
    // lane sub carries features sub and sub + 8 of its diagram (every lane of the group computes the same values)
    double o0 = 0.0, o1 = 0.0;
    auto put = [&](int idx, double v) { o0 = sub == idx ? v : o0; o1 = sub + 8 == idx ? v : o1; };
    put(1, (double)((k > 0 ? k : 0) - m));
    if (m > 0) {
        put(0, (double)m);
        auto fb = [=](int i) { return b[i]; };
        auto fd = [=](int i) { return d[i]; };
        auto fp = [=](int i) { return d[i] - b[i]; };
        double mean, sd;
        group8_mean_std(fb, m, sub, mean, sd); put(2, mean); put(3, sd);
        group8_mean_std(fd, m, sub, mean, sd); put(4, mean); put(5, sd);
        group8_mean_std(fp, m, sub, mean, sd); put(6, mean); put(7, sd);
        double mx = -INFINITY;
        for (int i = sub; i < m; i += 8) { const double pi = d[i] - b[i]; mx = pi > mx ? pi : mx; }
        { double o;
          o = dpp_f64<0xB1, 0xF>(mx); mx = o > mx ? o : mx;
          o = dpp_f64<0x4E, 0xF>(mx); mx = o > mx ? o : mx;
          o = dpp_f64<0x141, 0xF>(mx); mx = o > mx ? o : mx; }
        put(8, mx);
        const double tot = np_pairwise_group8(fp, m, sub);
        put(9, tot);
        if (m > 1 && tot > 0.0) {
            // pn = pers/sum; keep pn > 0 in order (utils.py:161-163): the terms go where the births were (term `at` <= row i,
            // and the rows of a later trip lie above every term written so far)
            int c = 0;
            for (int i0 = 0; i0 < m; i0 += 8) {
                const int i = i0 + sub;
                double pn = 0.0;
                if (i < m) pn = (d[i] - b[i]) / tot;
                const bool pos = i < m && pn > 0.0;
                const u32 bal = (u32)(__ballot(pos) >> (8 * grp)) & 0xffu;
                const int at = c + __popc(bal & ((1u << sub) - 1u));
                wave_sync();
                if (pos) b[at] = pn * log(pn + 1e-10);
                c += __popc(bal);
            }
            wave_sync();
            put(10, -np_pairwise_group8(fb, c, sub) / log((double)m + 1e-10));
        }
    }
    feat[(size_t)g * TDA_N_FEATURES + sub] = o0;
    if (sub + 8 < TDA_N_FEATURES) feat[(size_t)g * TDA_N_FEATURES + 8 + sub] = o1;
}

// ---------------------------------------------------------------------------------
// per (recording, band) aggregation: np.mean / np.std over the used windows
// out[seg][f*4 + {0,1,2,3}] = h0 mean, h0 std, h1 mean, h1 std   (v2:429-436)
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
aggregate_kernel(const double* __restrict__ f0, const double* __restrict__ f1, const int* __restrict__ seg_off,
                 int n_seg, double* __restrict__ out)
{
    const int seg = blockIdx.x;
    if (seg >= n_seg) return;
    const int lane = lane_id();
    if (lane >= 2 * TDA_N_FEATURES) return;
    const int h = lane / TDA_N_FEATURES, f = lane % TDA_N_FEATURES;
    const int s0 = seg_off[seg], s1 = seg_off[seg + 1];
    const int n = s1 - s0;
    const double* src = (h == 0 ? f0 : f1) + (size_t)s0 * TDA_N_FEATURES + f;
    double mean = 0.0, sd = 0.0;
    if (n > 0) {
        mean = np_pairwise_sum(src, n, TDA_N_FEATURES) / (double)n;
        // np.std = sqrt(mean(|x-mean|^2)), same pairwise tree evaluated on the fly
        auto sq = [=](int i) { const double z = src[(size_t)i * TDA_N_FEATURES] - mean; return z * z; };
        const double res = np_pairwise_fn(sq, 0, n);
        sd = sqrt(res / (double)n);
    }
    double* o = out + (size_t)seg * (4 * TDA_N_FEATURES) + f * 4 + h * 2;
    o[0] = mean;
    o[1] = sd;
}

// ---------------------------------------------------------------------------------
// np.nanmean over the windows of each (recording, band) group  (cmp:117-118, mvm:95)
// one lane per segment; sums follow numpy's pairwise tree over the non-NaN values
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
nanmean_kernel(const double* __restrict__ x, const int* __restrict__ seg_off, int n_seg, double* __restrict__ out)
{
    const int seg = blockIdx.x * 64 + threadIdx.x;
    if (seg >= n_seg) return;
    const int s0 = seg_off[seg], s1 = seg_off[seg + 1];
    // np.nanmean: NaNs replaced by 0, sum / count of non-NaN; all-NaN (or empty) -> NaN
    int cnt = 0;
    for (int i = s0; i < s1; ++i) cnt += (x[i] == x[i]) ? 1 : 0;
    auto val = [=](int i) { const double v = x[s0 + i]; return v == v ? v : 0.0; };
    const double sum = np_pairwise_fn(val, 0, s1 - s0);
    out[seg] = cnt > 0 ? sum / (double)cnt : __longlong_as_double(0x7ff8000000000000ll);
}

// ---------------------------------------------------------------------------------
// One row per (recording, band) group, the unit the GPUs exchange:
//   [ nanmean W_H0 (cmp:117), nanmean W_H1 (cmp:118), tau (cmp:83), n_windows, 44 aggregated EEG features (v2:429-436) ]
// = nanmean_kernel x 2 + aggregate_kernel + the row assembly in one launch (lanes 0..21 aggregate, 22/23 nanmean).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
recording_rows_kernel(const double* __restrict__ w0, const double* __restrict__ w1, const int* __restrict__ tau_seg,
                      const double* __restrict__ f0, const double* __restrict__ f1, const int* __restrict__ seg_off,
                      int n_seg, double* __restrict__ out, const int* __restrict__ status_a,
                      const int* __restrict__ status_b, int* __restrict__ seg_flags)
{
    const int seg = blockIdx.x;
    if (seg >= n_seg) return;
    const int lane = lane_id();
    const int s0 = seg_off[seg], s1 = seg_off[seg + 1];
    const int n = s1 - s0;
    double* row = out + (size_t)seg * (4 + 4 * TDA_N_FEATURES);
    if (lane < 2 * TDA_N_FEATURES) {
        const int h = lane / TDA_N_FEATURES, f = lane % TDA_N_FEATURES;
        const double* src = (h == 0 ? f0 : f1) + (size_t)s0 * TDA_N_FEATURES + f;
        double mean = 0.0, sd = 0.0;
        if (n > 0) {
            mean = np_pairwise_sum(src, n, TDA_N_FEATURES) / (double)n;
            auto sq = [=](int i) { const double z = src[(size_t)i * TDA_N_FEATURES] - mean; return z * z; };
            sd = sqrt(np_pairwise_fn(sq, 0, n) / (double)n);
        }
        row[4 + f * 4 + h * 2] = mean;
        row[4 + f * 4 + h * 2 + 1] = sd;
    } else if (lane < 2 * TDA_N_FEATURES + 2) {
        // cmp:90-91: a window whose Takens cloud has fewer than 3 points (or none at all) never reaches the
        // distances; np.nanmean then runs over the list of the windows that did (cmp:117-118).  No window left:
        // the reference drops the band (cmp:101-102), here the two distances are NaN.
        const double* x = lane == 2 * TDA_N_FEATURES ? w0 : w1;
        const int skip = TDA_WIN_DEGENERATE | TDA_WIN_TOO_LARGE;
        int m = 0, cnt = 0;
        for (int i = s0; i < s1; ++i) {
            if (status_b && (status_b[i] & skip)) continue;
            ++m;
            cnt += (x[i] == x[i]) ? 1 : 0;
        }
        // the j-th surviving window (the survivors keep their order, so the pairwise tree is numpy's)
        auto val = [=](int j) {
            int i = s0;
            if (status_b) { for (int seen = -1;; ++i) { if (!(status_b[i] & skip) && ++seen == j) break; } }
            else i = s0 + j;
            const double v = x[i];
            return v == v ? v : 0.0;
        };
        const double sum = np_pairwise_fn(val, 0, m);
        row[lane - 2 * TDA_N_FEATURES] = cnt > 0 ? sum / (double)cnt : __longlong_as_double(0x7ff8000000000000ll);
    } else if (lane == 2 * TDA_N_FEATURES + 2) {
        row[2] = (double)tau_seg[seg];
        row[3] = (double)n;
    } else if (lane == 2 * TDA_N_FEATURES + 3 && seg_flags) {
        int fl = 0;
        for (int i = s0; i < s1; ++i) fl |= (status_a ? status_a[i] : 0) | (status_b ? status_b[i] : 0);
        seg_flags[seg] = fl & ~TDA_WIN_DEGENERATE;          // every condition a caller has to act on (a degenerate cloud is a result)
    }
}

tda_status launch_recording_rows(tda_ctx* ctx, const double* w0, const double* w1, const int* tau_seg, const double* f0,
                                 const double* f1, const int* seg_off, int n_seg, double* out, const int* status_a,
                                 const int* status_b, int* seg_flags, hipStream_t st)
{
    if (n_seg == 0) return TDA_OK;
    hipLaunchKernelGGL(recording_rows_kernel, dim3(n_seg), dim3(64), 0, st, w0, w1, tau_seg, f0, f1, seg_off, n_seg, out,
                       status_a, status_b, seg_flags);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

// ---------------------------------------------------------------------------------
// The rows of the control experiment (mvm:86-95, 134-145): per EEG group
//   [ nanmean of the matched W_H1, nanmean of the mismatched W_H1, matched pairs, mismatched pairs ]
// from the two outputs of the cross Wasserstein launches.  The pairs of a group are its first n entries (mvm:89:
// n = min(len(eeg), len(audio))); the mean runs over exactly those, with nanmean_kernel's tree -- the entries
// without a pair never enter it (as zeros they would move the values to other accumulators of numpy's unrolled
// sum).  A pair whose solver status is set counts as NaN.  One lane per (group, side).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
cross_rows_kernel(const double* __restrict__ w_m, const int* __restrict__ st_m, const double* __restrict__ w_x,
                  const int* __restrict__ st_x, const int* __restrict__ seg_off, int n_seg, double* __restrict__ out,
                  const int* __restrict__ status_a, int* __restrict__ seg_flags)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int seg = t >> 1, side = t & 1;
    if (seg >= n_seg) return;
    const int s0 = seg_off[seg], s1 = seg_off[seg + 1];
    const double* x = side ? w_x : w_m;
    const int* st = side ? st_x : st_m;
    int n = 0, cnt = 0, fl = 0;
    for (int i = s0; i < s1; ++i) n += (st[i] & TDA_WIN_NO_PAIR) ? 0 : 1;
    for (int i = s0; i < s0 + n; ++i) {
        cnt += (st[i] == 0 && x[i] == x[i]) ? 1 : 0;
        fl |= st[i];
    }
    auto val = [=](int j) { const double v = x[s0 + j]; return (st[s0 + j] == 0 && v == v) ? v : 0.0; };
    const double sum = np_pairwise_fn(val, 0, n);
    double* row = out + (size_t)seg * 4;
    row[side] = cnt > 0 ? sum / (double)cnt : __longlong_as_double(0x7ff8000000000000ll);
    row[2 + side] = (double)n;
    if (seg_flags) {
        // both sides of a group sit in neighbouring lanes of one wave
        if (status_a && side == 0) for (int i = s0; i < s1; ++i) fl |= status_a[i];
        fl |= __shfl_xor(fl, 1, 64);
        if (side == 0) seg_flags[seg] = fl & ~(TDA_WIN_NO_PAIR | TDA_WIN_DEGENERATE);
    }
}

tda_status launch_cross_rows(tda_ctx* ctx, const double* w_m, const int* st_m, const double* w_x, const int* st_x,
                             const int* seg_off, int n_seg, double* out, const int* status_a, int* seg_flags, hipStream_t st)
{
    if (n_seg == 0) return TDA_OK;
    hipLaunchKernelGGL(cross_rows_kernel, dim3((2 * n_seg + 63) / 64), dim3(64), 0, st, w_m, st_m, w_x, st_x, seg_off, n_seg,
                       out, status_a, seg_flags);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_nanmean(tda_ctx* ctx, const double* x, const int* seg_off, int n_seg, double* out, hipStream_t st)
{
    if (n_seg == 0) return TDA_OK;
    hipLaunchKernelGGL(nanmean_kernel, dim3((n_seg + 63) / 64), dim3(64), 0, st, x, seg_off, n_seg, out);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

// ---------------------------------------------------------------------------------
// Spearman correlation of two feature time series per (recording, band) group:
// scripts/tda_eeg_audio_comparison.py:104-114 -> scipy.stats.spearmanr = Pearson correlation
// (np.corrcoef) of the average ranks.  x, y: (n_total, ld) rows = windows; column `col`.
// r = 0 when the group has < 5 windows or either series has np.std <= 1e-10 (cmp:110-114).
// One thread per (group, column); groups are tiny (<= 15 windows in the reference).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
spearman_kernel(const double* __restrict__ x, const double* __restrict__ y, int ld, const int* __restrict__ cols,
                int n_cols, const int* __restrict__ seg_off, int n_seg, double* __restrict__ r_out)
{
    const int seg = blockIdx.x;
    const int ci = threadIdx.x;
    if (seg >= n_seg || ci >= n_cols) return;
    const int col = cols[ci];
    const int s0 = seg_off[seg], n = seg_off[seg + 1] - s0;
    const double* xa = x + (size_t)s0 * ld + col;
    const double* ya = y + (size_t)s0 * ld + col;
    double r = 0.0;
    if (n >= 5) {
        auto fx = [=](int i) { return xa[(size_t)i * ld]; };
        auto fy = [=](int i) { return ya[(size_t)i * ld]; };
        const double mx = np_pairwise_fn(fx, 0, n) / n, my = np_pairwise_fn(fy, 0, n) / n;
        auto vx = [=](int i) { const double z = xa[(size_t)i * ld] - mx; return z * z; };
        auto vy = [=](int i) { const double z = ya[(size_t)i * ld] - my; return z * z; };
        const double sx = sqrt(np_pairwise_fn(vx, 0, n) / n), sy = sqrt(np_pairwise_fn(vy, 0, n) / n);
        if (sx > 1e-10 && sy > 1e-10) {
            // average ranks (scipy.stats.rankdata, method="average"), centred: sum of ranks = n(n+1)/2
            const double mr = 0.5 * (double)(n + 1);
            double sxx = 0.0, syy = 0.0, sxy = 0.0;
            for (int i = 0; i < n; ++i) {
                const double xi = xa[(size_t)i * ld], yi = ya[(size_t)i * ld];
                int lx = 0, ex = 0, ly = 0, ey = 0;
                for (int j = 0; j < n; ++j) {
                    const double xj = xa[(size_t)j * ld], yj = ya[(size_t)j * ld];
                    lx += xj < xi; ex += xj == xi; ly += yj < yi; ey += yj == yi;
                }
                const double rx = (double)lx + 0.5 * (double)(ex + 1) - mr;
                const double ry = (double)ly + 0.5 * (double)(ey + 1) - mr;
                sxx += rx * rx; syy += ry * ry; sxy += rx * ry;
            }
            r = (sxy / sqrt(sxx)) / sqrt(syy);
            if (r > 1.0) r = 1.0;
            if (r < -1.0) r = -1.0;
        }
    }
    r_out[(size_t)seg * n_cols + ci] = r;
}

tda_status launch_spearman(tda_ctx* ctx, const double* x, const double* y, int ld, const int* cols, int n_cols,
                           const int* seg_off, int n_seg, double* r_out, hipStream_t st)
{
    if (n_seg == 0 || n_cols == 0) return TDA_OK;
    if (n_cols > 64) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "at most 64 columns");
    hipLaunchKernelGGL(spearman_kernel, dim3(n_seg), dim3(64), 0, st, x, y, ld, cols, n_cols, seg_off, n_seg, r_out);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

// ---------------------------------------------------------------------------------
// Temporal correlation of the H1 feature time series of a step (cmp:90-91,104-114): per (recording, band) group and
// feature column, Spearman r AND its two-sided p-value of the audio series against the EEG series over the windows that
// reached the distances.  Unlike spearman_kernel it takes the per-window matrices of a step as they are: the windows
// cmp:90-91 skips are left out here, by the rule and the constants of recording_rows_kernel.
//   m = survivors;  m == 0: NaN, NaN (the reference drops the band, cmp:101-102);  m < 5 or np.std of a series
//   <= 1e-10: 0, 1 (cmp:110-114);  otherwise r as spearman_kernel on the compacted series, bit for bit, and
//   p = I_{1-r^2}((m-2)/2, 1/2).
// One wavefront per group.  Up to TC_CAP survivors (numpy's pairwise leaf; the reference has <= 15, every window of the
// corpus <= 89) are compacted into LDS with a ballot and a prefix popcount, all columns of a trip at once; a longer
// group is read in place from global memory, the skipped windows stepped over.  Either way the series sit behind one
// accessor: slot k (valid or not), and for the guard's sums the j-th survivor.
//   * guard: every lane evaluates the same four sums per column with numpy's pairwise tree (same-address reads)
//   * ranks: lane i owns slot i (chunks of 64) and walks all slots j -- same-address reads again, a broadcast.  The
//     centred average ranks are multiples of 1/2, their products multiples of 1/4 and their sums (<= m^3 / 4) stay
//     below 2^53 quarters for m < 2^17: the three sums are EXACT in float64 in any order, so the per-lane partial sums and the butterfly give
//     the bits spearman_kernel's sequential loop gives
//   * p: lane c evaluates column c's p-value (the serial part: a product of <= m/2 factors and a continued fraction)
// No allocation, no host round trip, fixed launch shape: it can be captured into a graph.
// ---------------------------------------------------------------------------------
#define TC_CAP 128
#define TC_COLS 8

struct TcLds {                     // compacted survivors in LDS: every slot valid, survivor j = slot j
    const double* xs; const double* ys; int m;
    __device__ __forceinline__ int slots() const { return m; }
    __device__ __forceinline__ bool valid(int) const { return true; }
    __device__ __forceinline__ double x(int k) const { return xs[k]; }
    __device__ __forceinline__ double y(int k) const { return ys[k]; }
    __device__ __forceinline__ int survivor(int j) { return j; }
};
struct TcGlobal {                  // the group in place: slot k = window k, survivor j found by a cursor
    const double* xa; const double* ya; int ld; const int* st; int n;
    int cur = -1, seen = -1;       // slot `cur` is survivor number `seen`
    __device__ __forceinline__ int slots() const { return n; }
    __device__ __forceinline__ bool valid(int k) const { return !(st && (st[k] & (TDA_WIN_DEGENERATE | TDA_WIN_TOO_LARGE))); }
    __device__ __forceinline__ double x(int k) const { return xa[(size_t)k * ld]; }
    __device__ __forceinline__ double y(int k) const { return ya[(size_t)k * ld]; }
    // numpy's pairwise tree asks for its terms in rising order, so the cursor only ever steps forward within a sum
    __device__ __forceinline__ int survivor(int j)
    {
        if (j < seen) { cur = -1; seen = -1; }
        while (seen < j) { ++cur; seen += valid(cur) ? 1 : 0; }
        return cur;
    }
};

// np.sum of f(0) .. f(m-1), the same sum in every lane of the wave: no call, no private array
template <class F>
__device__ __forceinline__ double tc_sum(const F& f, int m)
{
    return m <= 128 ? np_pairwise_leaf(f, 0, m) : np_pairwise_split_uniform(f, 0, m);
}

// r of one column; 0 under the guard of cmp:110 (m >= 5 is the caller's)
template <class A>
__device__ __forceinline__ double tc_column(A acc, int m, int lane)
{
    auto fx = [&](int j) { return acc.x(acc.survivor(j)); };
    auto fy = [&](int j) { return acc.y(acc.survivor(j)); };
    const double mx = tc_sum(fx, m) / m, my = tc_sum(fy, m) / m;
    auto vx = [&](int j) { const double z = acc.x(acc.survivor(j)) - mx; return z * z; };
    auto vy = [&](int j) { const double z = acc.y(acc.survivor(j)) - my; return z * z; };
    const double sx = sqrt(tc_sum(vx, m) / m), sy = sqrt(tc_sum(vy, m) / m);
    if (!(sx > 1e-10 && sy > 1e-10)) return 0.0;
    // average ranks (scipy.stats.rankdata, method="average"), centred: sum of ranks = m(m+1)/2
    const double mr = 0.5 * (double)(m + 1);
    const int K = acc.slots();
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int i0 = 0; i0 < K; i0 += 64) {
        const int i = i0 + lane;
        if (i < K && acc.valid(i)) {
            const double xi = acc.x(i), yi = acc.y(i);
            int lx = 0, ex = 0, ly = 0, ey = 0;
            for (int j = 0; j < K; ++j) {
                if (!acc.valid(j)) continue;
                const double xj = acc.x(j), yj = acc.y(j);
                lx += xj < xi; ex += xj == xi; ly += yj < yi; ey += yj == yi;
            }
            const double rx = (double)lx + 0.5 * (double)(ex + 1) - mr;
            const double ry = (double)ly + 0.5 * (double)(ey + 1) - mr;
            sxx += rx * rx; syy += ry * ry; sxy += rx * ry;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sxx += __shfl_xor(sxx, off, 64); syy += __shfl_xor(syy, off, 64); sxy += __shfl_xor(sxy, off, 64);
    }
    double r = (sxy / sqrt(sxx)) / sqrt(syy);
    if (r > 1.0) r = 1.0;
    if (r < -1.0) r = -1.0;
    return r;
}

// Continued fraction of the incomplete beta function, modified Lentz evaluation (Numerical Recipes 6.4): converges in
// O(sqrt(max(a, b))) trips for x < (a + 1) / (a + b + 2).
__device__ __forceinline__ double tc_betacf(double a, double b, double x)
{
    const double tiny = 1e-300, eps = 3e-16;            // (one ulp of 1 and a little: del may settle an ulp off 1)
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int i = 1; i <= 20000; ++i) {
        const double i2 = 2.0 * i;
        double aa = i * (b - i) * x / ((qam + i2) * (a + i2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + i) * (qab + i) * x / ((a + i2) * (qap + i2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= eps) break;
    }
    return h;
}
// Two-sided p-value of a correlation r of m pairs under Student's t with m - 2 degrees of freedom (what
// scipy.stats.spearmanr reports): I_x(a, 1/2) with x = 1 - r^2, a = (m - 2) / 2.  a is an integer or a half-integer, so
// 1 / B(a, 1/2) is a finite product from 1 / B(1/2, 1/2) = 1 / pi or 1 / B(1, 1/2) = 1 / 2; (1 - x)^(1/2) = |r|.
// Exactly 0 at r = +-1 and exactly 1 at r = 0.
__device__ __forceinline__ double tc_pvalue(double r, int m)
{
    const double x = (1.0 + r) * (1.0 - r), y = r * r;
    if (!(x > 0.0)) return 0.0;
    if (!(y > 0.0)) return 1.0;
    const int k = m - 2;
    const double a = 0.5 * (double)k;
    double ib = (k & 1) ? 0.31830988618379067154 : 0.5;
    for (double t = (k & 1) ? 0.5 : 1.0; t < a; t += 1.0) ib *= (t + 0.5) / t;
    const double bt = ib * fabs(r) * exp(a * log(x));
    double p;
    if (x < (a + 1.0) / (a + 2.5)) p = bt * tc_betacf(a, 0.5, x) / a;
    else p = 1.0 - bt * tc_betacf(0.5, a, y) / 0.5;
    return p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p);
}

__global__ void __launch_bounds__(64)
temporal_corr_kernel(const double* __restrict__ fa, const double* __restrict__ fe, int ld, const int* __restrict__ cols,
                     int n_cols, const int* __restrict__ seg_off, int n_seg, const int* __restrict__ status_b,
                     double* __restrict__ out)
{
    __shared__ double sx[TC_COLS][TC_CAP], sy[TC_COLS][TC_CAP];
    const int seg = blockIdx.x;
    if (seg >= n_seg) return;
    const int lane = lane_id();
    const int s0 = uni(seg_off[seg]), n = uni(seg_off[seg + 1]) - s0;
    const int* st = status_b ? status_b + s0 : nullptr;
    const int skip = TDA_WIN_DEGENERATE | TDA_WIN_TOO_LARGE;
    int m = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        m += __popcll(__ballot(i < n && !(st && (st[i] & skip))));
    }
    double* row = out + (size_t)seg * 2 * n_cols;
    if (m < 5) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int c = lane; c < 2 * n_cols; c += 64) row[c] = m == 0 ? nan : (double)(c & 1);
        return;
    }
    for (int c0 = 0; c0 < n_cols; c0 += TC_COLS) {
        const int nc = n_cols - c0 < TC_COLS ? n_cols - c0 : TC_COLS;
        double r_mine = 0.0;                                           // lane c: r of column c0 + c
        if (m <= TC_CAP) {
            int base = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                const bool alive = i < n && !(st && (st[i] & skip));
                const u64 bal = __ballot(alive);
                const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
                if (alive) {
                    const double* pa = fa + (size_t)(s0 + i) * ld;
                    const double* pe = fe + (size_t)(s0 + i) * ld;
                    for (int c = 0; c < nc; ++c) { const int col = cols[c0 + c]; sx[c][pos] = pa[col]; sy[c][pos] = pe[col]; }
                }
                base += __popcll(bal);
            }
            wave_sync();
            for (int c = 0; c < nc; ++c) {
                const double r = tc_column(TcLds{sx[c], sy[c], m}, m, lane);
                r_mine = lane == c ? r : r_mine;
            }
            wave_sync();                                               // (the next trip overwrites the series)
        } else {
            for (int c = 0; c < nc; ++c) {
                const int col = cols[c0 + c];
                const double r = tc_column(TcGlobal{fa + (size_t)s0 * ld + col, fe + (size_t)s0 * ld + col, ld, st, n}, m, lane);
                r_mine = lane == c ? r : r_mine;
            }
        }
        if (lane < nc) {
            row[2 * (c0 + lane)] = r_mine;
            row[2 * (c0 + lane) + 1] = tc_pvalue(r_mine, m);
        }
    }
}

tda_status launch_temporal_corr(tda_ctx* ctx, const double* fa, const double* fe, int ld, const int* cols, int n_cols,
                                const int* seg_off, int n_seg, const int* status_b, double* out, hipStream_t st)
{
    if (n_seg == 0 || n_cols == 0) return TDA_OK;
    hipLaunchKernelGGL(temporal_corr_kernel, dim3(n_seg), dim3(64), 0, st, fa, fe, ld, cols, n_cols, seg_off, n_seg,
                       status_b, out);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

// ---------------------------------------------------------------------------------
tda_status launch_tau(tda_ctx* ctx, const double* win, int n_win, int n_t, int max_lag, int* tau, hipStream_t st)
{
    if (n_win == 0) return TDA_OK;
    if (n_t < 2 || n_t > 8192) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "n_t must be in [2,8192]");
    hipLaunchKernelGGL(tau_kernel, dim3(n_win), dim3(64), (size_t)n_t * 8, st, win, n_win, n_t, max_lag, tau,
                       (const int*)nullptr, (int*)nullptr);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_tau_segments(tda_ctx* ctx, const double* win, const int* seg_off, int n_seg, int n_t, int max_lag,
                               int* tau_seg, int* tau_win, hipStream_t st)
{
    if (n_seg == 0) return TDA_OK;
    if (n_t < 2 || n_t > 8192) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "n_t must be in [2,8192]");
    hipLaunchKernelGGL(tau_kernel, dim3(n_seg), dim3(64), (size_t)n_t * 8, st, win, n_seg, n_t, max_lag, tau_seg, seg_off,
                       tau_win);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_diagram_finish(tda_ctx* ctx, const tda_diagram_set* sets, int n_sets, int n_dgm, hipStream_t st)
{
    if (n_dgm == 0 || n_sets == 0) return TDA_OK;
    if (n_sets < 0 || n_sets > 4) TDA_FAIL(ctx, TDA_ERR_INVALID, "1 to 4 diagram sets per launch");
    DiagramSets S;
    int cap = 1;
    for (int i = 0; i < 4; ++i) {
        const bool on = i < n_sets;
        S.rows[i] = on ? sets[i].rows : nullptr; S.cnt[i] = on ? sets[i].cnt : nullptr;
        S.cap[i] = on ? sets[i].cap : 0; S.order[i] = on ? sets[i].order : 0; S.feat[i] = on ? sets[i].feat : nullptr;
        if (on) {
            if (!sets[i].rows || !sets[i].cnt) TDA_FAIL(ctx, TDA_ERR_INVALID, "null diagram set");
            if (sets[i].cap < 1 || sets[i].cap > 4096) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "diagram capacity must be in [1,4096]");
            cap = sets[i].cap > cap ? sets[i].cap : cap;
        }
    }
    S.n_sets = n_sets;
    const long long n_all = (long long)n_sets * n_dgm;
    // small diagrams first, then whatever is larger with slices of the full capacity.  TDA_SCHEME_LISTS: the packed kernel,
    // and the wide launch over the list of the diagrams it left; TDA_SCHEME_GRID: the one-wave-per-diagram kernel with
    // slices of 64 rows, and the wide launch over the whole batch; TDA_SCHEME_ONE (or TDA_FINISH_ONE_LAUNCH): that alone
    static const bool one_launch = getenv("TDA_FINISH_ONE_LAUNCH") != nullptr;
    int scheme = one_launch ? TDA_SCHEME_ONE : ctx->launch_scheme;
    int nw = FIN_WAVES;                                  // diagrams per workgroup: fewer when the slices are large
    while (nw > 1 && (size_t)cap * 4 * 8 * nw > 32 * 1024) nw >>= 1;
    const size_t lds = (size_t)cap * 4 * 8 * nw;
    if (lds > 48 * 1024 && (cap > FINP_ROWS || scheme != TDA_SCHEME_LISTS)) {
        TDA_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(diagram_finish_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        TDA_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(diagram_finish_list_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    if (scheme == TDA_SCHEME_LISTS) {
        int* list = nullptr;
        if (cap > FINP_ROWS) {
            int slot = -1;
            if (n_all <= INT_MAX) { const tda_status rc = stream_lists_take(ctx, (int)n_all, st, &slot); if (rc != TDA_OK) return rc; }
            if (slot < 0) scheme = TDA_SCHEME_GRID;      // no list of that size (see stream_lists_take)
            else list = ctx->fin_list[slot];
        }
        if (scheme == TDA_SCHEME_LISTS) {
            const long long waves = (long long)n_sets * ((n_dgm + 7) / 8);
            hipLaunchKernelGGL(diagram_finish_packed_kernel, dim3((unsigned)((waves + FINP_WAVES - 1) / FINP_WAVES)),
                               dim3(64 * FINP_WAVES), (size_t)FINP_WAVES * 8 * FINP_STRIDE * 8, st, S, n_dgm, list);
            if (list) {
                const long long wgs = (n_all + nw - 1) / nw;
                hipLaunchKernelGGL(diagram_finish_list_kernel, dim3((unsigned)(wgs < 256 ? wgs : 256)), dim3(64 * nw), lds, st, S,
                                   n_dgm, cap, FINP_ROWS, list);
            }
            TDA_HIP(ctx, hipGetLastError());
            return TDA_OK;
        }
    }
    int k_lo = INT_MIN;
    if (cap > 64 && scheme == TDA_SCHEME_GRID) {
        hipLaunchKernelGGL(diagram_finish_kernel, dim3((unsigned)((n_all + FIN_WAVES - 1) / FIN_WAVES)), dim3(64 * FIN_WAVES),
                           (size_t)64 * 4 * 8 * FIN_WAVES, st, S, n_dgm, 64, k_lo);
        k_lo = 64;
    }
    hipLaunchKernelGGL(diagram_finish_kernel, dim3((unsigned)((n_all + nw - 1) / nw)), dim3(64 * nw), lds, st, S, n_dgm, cap, k_lo);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_features(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm, int cap, double* feat,
                           hipStream_t st)
{
    if (cap < 1 || cap > 2048) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "diagram capacity must be in [1,2048]");
    tda_diagram_set one{const_cast<double*>(dgm), cnt, cap, 0, feat};
    return launch_diagram_finish(ctx, &one, 1, n_dgm, st);
}

tda_status launch_aggregate(tda_ctx* ctx, const double* f0, const double* f1, const int* seg_off, int n_seg,
                            double* out, hipStream_t st)
{
    if (n_seg == 0) return TDA_OK;
    hipLaunchKernelGGL(aggregate_kernel, dim3(n_seg), dim3(64), 0, st, f0, f1, seg_off, n_seg, out);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
