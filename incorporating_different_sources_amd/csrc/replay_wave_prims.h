#pragma once
// replay_wave_prims.h - what the backtest replay (backtest_replay.hip) and its summary (replay_summary.hip) share: the fixed
// 64-lane trees of their sums, maxima and minima, the NaN helpers and the wave-uniform values.  One definition each.
#include "posterior_device_prims.h"

namespace {

// Sums of N values at once, every lane gets them: four DPP rotations inside each row of 16 lanes (no LDS crossbar), then the
// four row sums through v_readlane as (S0 + S1) + (S2 + S3).  A fixed tree; every lane ends with the same bits.  All 64 lanes
// are active wherever these are called (the control flow around them is wave-uniform).
template <int N>
__device__ __forceinline__ void wave_sums(double (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_row_ror<8>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_row_ror<4>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_row_ror<2>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += dpp_row_ror<1>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i)
        v[i] = (readlane_d(v[i], 0) + readlane_d(v[i], 16)) + (readlane_d(v[i], 32) + readlane_d(v[i], 48));
}

__device__ __forceinline__ double wave_sum(double x) {
    double v[1] = {x};
    wave_sums(v);
    return v[0];
}

// selections: the result is one of the inputs, whatever the order
__device__ __forceinline__ double pick_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double pick_min(double a, double b) { return b < a ? b : a; }

__device__ __forceinline__ double wave_max(double v) {
    v = pick_max(v, dpp_row_ror<8>(v));
    v = pick_max(v, dpp_row_ror<4>(v));
    v = pick_max(v, dpp_row_ror<2>(v));
    v = pick_max(v, dpp_row_ror<1>(v));
    return pick_max(pick_max(readlane_d(v, 0), readlane_d(v, 16)), pick_max(readlane_d(v, 32), readlane_d(v, 48)));
}

__device__ __forceinline__ double wave_min(double v) {
    v = pick_min(v, dpp_row_ror<8>(v));
    v = pick_min(v, dpp_row_ror<4>(v));
    v = pick_min(v, dpp_row_ror<2>(v));
    v = pick_min(v, dpp_row_ror<1>(v));
    return pick_min(pick_min(readlane_d(v, 0), readlane_d(v, 16)), pick_min(readlane_d(v, 32), readlane_d(v, 48)));
}

__device__ __forceinline__ bool is_nan(double x) { return x != x; }
__device__ __forceinline__ double nan_to_zero(double x) { return x != x ? 0.0 : x; }

// a value every lane holds alike, for the scalar unit
__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ long long uniform(long long x) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)x & 0xffffffffull));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)x >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double uniform(double x) { return __longlong_as_double(uniform(__double_as_longlong(x))); }

}  // namespace
