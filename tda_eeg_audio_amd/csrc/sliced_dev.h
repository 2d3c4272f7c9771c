// sliced_dev.h -- what the sliced Wasserstein kernels share: the bitonic network on 64 V doubles per wave, the butterfly
// sum over the lanes and the cleaning of one diagram into LDS.  Included by sliced.hip (the pair kernel) and
// sliced_matrix.hip (the prepare kernel sorts with the same network; the prepared kernels add with the same butterfly).
// The code is sliced.hip's, moved, not changed: tools/isa_diff.py --files sliced --match sliced_kernel says `same`.
#ifndef TDA_SLICED_DEV_H
#define TDA_SLICED_DEV_H
#include "common.h"

#pragma clang fp contract(off)

#define SW_WAVES 4

// the value of lane ^ J (both halves of a double travel the same way)
template <int J>
__device__ __forceinline__ int sw_xor_i32(int v)
{
    if constexpr (J == 1) return __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
    else if constexpr (J == 2) return __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    else if constexpr (J < 32) return __builtin_amdgcn_ds_swizzle(v, (J << 10) | 0x1f);           // bit mode: and 31, or 0, xor J
    else return __builtin_amdgcn_ds_bpermute((lane_id() ^ 32) << 2, v);
}
template <int J>
__device__ __forceinline__ double sw_xor_f64(double v)
{
    return __hiloint2double(sw_xor_i32<J>(__double2hiint(v)), sw_xor_i32<J>(__double2loint(v)));
}

// the steps j = J, J/2, .., 1 of the merge of blocks of K elements
template <int V, int K, int J>
__device__ __forceinline__ void sw_merge(double (&x)[V], int lane)
{
    if constexpr (J >= 64) {
        constexpr int RJ = J / 64, RK = K / 64;
#pragma unroll
        for (int r = 0; r < V; ++r) {
            if ((r & RJ) != 0) continue;
            const bool desc = (r & RK) != 0;
            const double a = x[r], b = x[r | RJ];
            const bool sw = desc ? a < b : b < a;
            x[r] = sw ? b : a;
            x[r | RJ] = sw ? a : b;
        }
    } else {
        const bool upper = (lane & J) != 0;
#pragma unroll
        for (int r = 0; r < V; ++r) {
            const bool desc = K < 64 ? (lane & K) != 0 : (r & (K / 64)) != 0;
            const bool keep_min = upper == desc;
            const double v = x[r], o = sw_xor_f64<J>(v);
            const bool take = keep_min ? o < v : o > v;      // (the partner decides the same swap from its side)
            x[r] = take ? o : v;
        }
    }
    if constexpr (J > 1) sw_merge<V, K, J / 2>(x, lane);
}
template <int V, int K>
__device__ __forceinline__ void sw_sort(double (&x)[V], int lane)
{
    sw_merge<V, K, K / 2>(x, lane);
    if constexpr (K < 64 * V) sw_sort<V, 2 * K>(x, lane);
}

// the sum over the 64 lanes, the same bits on every lane (a + b == b + a at every level)
__device__ __forceinline__ double sw_wave_sum(double v)
{
    v = v + sw_xor_f64<1>(v);
    v = v + sw_xor_f64<2>(v);
    v = v + sw_xor_f64<4>(v);
    v = v + sw_xor_f64<8>(v);
    v = v + sw_xor_f64<16>(v);
    v = v + sw_xor_f64<32>(v);
    return v;
}

// finite rows of one diagram into LDS as (b, d) pairs with their h, order kept; none: {(0, 0)}.  At most `room` rows are
// written; the count that is returned goes on (a pair with more than that is refused by the caller).  One wave.
__device__ __forceinline__ int sw_load(const double* __restrict__ src, int k, int room, double* pts, double* hs)
{
    const int lane = lane_id();
    int m = 0;
    for (int i0 = 0; i0 < k; i0 += 64) {
        const int i = i0 + lane;
        double b = 0, d = 0; bool fin = false;
        if (i < k) { b = src[2 * i]; d = src[2 * i + 1]; fin = isfinite(b) && isfinite(d); }
        const u64 bal = __ballot(fin);
        const int pos = m + __popcll(bal & ((1ull << lane) - 1ull));
        if (fin && pos < room) { pts[2 * pos] = b; pts[2 * pos + 1] = d; hs[pos] = 0.5 * (b + d); }
        m += __popcll(bal);
    }
    if (m == 0) {
        if (lane == 0) { pts[0] = 0.0; pts[1] = 0.0; hs[0] = 0.5 * (0.0 + 0.0); }
        m = 1;
    }
    return m;
}
#endif
