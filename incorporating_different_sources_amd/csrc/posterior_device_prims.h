#pragma once
// posterior_device_prims.h - the device primitives every kernel file shares: compile-time loops, lane exchange (DPP,
// v_readlane, shuffles), reductions, the reciprocal square root of the pivot chains and the upper-triangle pair decode.
// One definition each; the kernel files keep only what is theirs alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "posterior_kernels.h"

typedef double d4 __attribute__((ext_vector_type(4)));

namespace {

template <int V> using ic = std::integral_constant<int, V>;

// compile-time loop: f(ic<B>) ... f(ic<E-1>) (tile coordinates and register indices must be constants)
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) { f(ic<B>{}); static_for<B + 1, E>(f); }
}

__device__ __forceinline__ double readlane_d(double v, int lane) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// rotate right by N lanes inside each row of 16 lanes (DPP row_ror:N) - no LDS crossbar involved
template <int N>
__device__ __forceinline__ double dpp_row_ror(double v) {
    // every lane of a row_ror has a source lane: no "old" value is needed (mov_dpp leaves it undefined)
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x120 + N, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x120 + N, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// sum over the 16 lanes that share lane>>4 (one MFMA row group); every lane gets the sum
__device__ __forceinline__ double rowgroup_sum16(double v) {
    v += dpp_row_ror<8>(v);
    v += dpp_row_ror<4>(v);
    v += dpp_row_ror<2>(v);
    v += dpp_row_ror<1>(v);
    return v;
}

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// 1/sqrt(d) from the v_rsq_f64 seed (23 good bits) by ONE third-order step, y (1 + e/2 + 3 e^2/8) with
// e = 1 - d y^2: the error term is O(e^3) ~ 2^-68.  Six instructions on a chain of five (rsqrt_nr: nine on
// seven) - the pivot chain of the factorisation pays for both.
__device__ __forceinline__ double rsqrt_cubic(double d) {
    const double y = __builtin_amdgcn_rsq(d);
    const double e = fma(-(d * y), y, 1.0);
    const double u = fma(e, 0.375, 0.5);
    return fma(y * e, u, y);
}

// upper-triangle pair p -> (a, b), a <= b < n, row-major
__device__ __forceinline__ void pair_decode(int p, int n, int& a, int& b) {
    int i = 0, rem = p;
    while (rem >= n - i) { rem -= n - i; ++i; }
    a = i; b = i + rem;
}

}  // namespace
