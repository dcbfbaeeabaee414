// pgi_reduce.hpp -- the deterministic floating-point reductions of the averaging and bundle solvers (device code).
// "Same input, same bits" rests on every sum having ONE documented association; the solvers share these and write none of
// their own.  (wave_sum_exact of pgi_device.hpp belongs to a different family: its summands are pre-rounded so that any order
// gives the same bits, and it adds in another order -- rows of 16 first -- than wave_sum below.  Do not exchange them.)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pgi {
#define PGI_RDEV __device__ __forceinline__

// Sum over the 64 lanes of a wavefront by the xor tree 32, 16, ..., 1: the same order on every call, the sum in every lane.
PGI_RDEV double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// Sum over groups of LANES neighbouring lanes (a view's row shared by LANES lanes) by the xor tree 1, 2, ..., LANES / 2,
// per component; the sums in every lane of the group.  Needs every lane of the wavefront.
template <int NC, int LANES>
PGI_RDEV void row_lanes_sum(double* v) {
#pragma unroll
    for (int m = 1; m < LANES; m <<= 1)
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] += __shfl_xor(v[c], m);
}
template <int NC>
PGI_RDEV void row_lanes_sum(double* v, uint32_t lanes) {  // the same tree for a group size known at run time (a power of two)
    for (uint32_t m = 1; m < lanes; m <<= 1)
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] += __shfl_xor(v[c], (int)m);
}

// Thread tid's share of a sum over n records of `stride` doubles (NC leading components each): records tid, tid + NTHREADS,
// ... in that order.  The caller combines the threads' shares with wave_sum or block_tree_sum.
template <int NC, int NTHREADS>
PGI_RDEV void strided_sum(const double* __restrict__ part, uint32_t n, uint32_t stride, int tid, double* v) {
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = 0.0;
    for (uint32_t b = (uint32_t)tid; b < n; b += NTHREADS)
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] += part[stride * (size_t)b + c];
}

template <int NTHREADS>
PGI_RDEV double strided_sum(const double* __restrict__ part, uint32_t n, uint32_t stride, int tid) {  // one component
    double v;
    strided_sum<1, NTHREADS>(part, n, stride, tid, &v);
    return v;
}

// Block-wide sum of NC values per thread with the association "entry t takes entry t + s, s = BLOCK / 2, ..., 1", per
// component; every thread returns the block's sums.  red: NC * BLOCK doubles of LDS.  Two bodies, one association:
//   TreeInLds      every step through LDS, a barrier per step;
//   TreeInWave0    the steps down to s = 64 through LDS, the lower six as shuffles inside wavefront 0 (lane t + lane t + s
//                  for t < s is the same addition): at 256 threads two barriers before the result instead of nine, for
//                  the kernels on the critical path of a PCG iteration.
struct TreeInLds {};
struct TreeInWave0 {};
template <int NC, int BLOCK>
PGI_RDEV void block_tree_sum(double* v, double* red, int tid, TreeInLds = {}) {
#pragma unroll
    for (int c = 0; c < NC; ++c) red[BLOCK * c + tid] = v[c];
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int c = 0; c < NC; ++c) red[BLOCK * c + tid] += red[BLOCK * c + tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = red[BLOCK * c];
    __syncthreads();
}
template <int NC, int BLOCK>
PGI_RDEV void block_tree_sum(double* v, double* red, int tid, TreeInWave0) {
    static_assert(BLOCK >= 128, "the wavefront-0 tail takes over at s = 64");
#pragma unroll
    for (int c = 0; c < NC; ++c) red[BLOCK * c + tid] = v[c];
    __syncthreads();
#pragma unroll
    for (int s = BLOCK / 2; s > 64; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int c = 0; c < NC; ++c) red[BLOCK * c + tid] += red[BLOCK * c + tid + s];
        }
        __syncthreads();
    }
    if (tid < 64) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double x = red[BLOCK * c + tid] + red[BLOCK * c + tid + 64];
#pragma unroll
            for (int sft = 32; sft >= 1; sft >>= 1) x += __shfl_down(x, sft);  // lane t (< sft) gets x_t + x_{t + sft}
            if (tid == 0) red[BLOCK * c] = x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = red[BLOCK * c];
    __syncthreads();
}
template <int BLOCK>
PGI_RDEV double block_tree_sum(double v, double* red, int tid) {  // one component, TreeInLds
    block_tree_sum<1, BLOCK>(&v, red, tid);
    return v;
}

// ---- the pair of the spanning-tree kernel (1024 threads).  A DIFFERENT association from block_tree_sum: the wavefronts'
// xor-tree sums, then those 16 values added serially.  red: 16 doubles of LDS.
PGI_RDEV double block_wave_sum_1024(double v, double* red, int tid) {  // returned to all threads
    v = wave_sum(v);
    __syncthreads();  // previous use of red is over
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += red[i];
    return s;
}
// exclusive prefix (in thread order) of one value per thread
PGI_RDEV double block_prefix_1024(double v, double* red, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    double x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    __syncthreads();  // previous use of red is over
    if (lane == 63) red[wv] = x;
    __syncthreads();
    double before = 0.0;
    for (int i = 0; i < wv; ++i) before += red[i];
    return before + (x - v);
}
}  // namespace pgi
