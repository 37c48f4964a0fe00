// The selection idioms of the decoders' device steps (beam.hip, contrastive.hip), one definition each: the candidate order, the running
// softmax pair, the sorted register list, the block arg-max round and what is built on it.  All blocks here are whole waves of 64 lanes.
#pragma once
#include "common.hip.h"

namespace CC_NS {

constexpr int SEL_NONE = 0x7fffffff;      // the index of "no candidate": loses every comparison, never a real flat index or token id

// the candidate order: higher value first, ties to the lower index
__device__ __forceinline__ bool cand_better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// ---- running softmax pair -------------------------------------------------------------------------------------------------------------
// (max, sum of exp(x - max)) of the values seen so far; the sum is rescaled when the max moves, so a row is read once.  -inf values (banned
// tokens, constrain.hip) may come first: nothing is added while the max is -inf, so there is no -inf - -inf.  k_contrastive_topk uses it;
// k_beam_rowstats (beam.hip) keeps the same arithmetic written out, because it compiles to slower code through this struct.
struct SoftmaxPair {
    float m = -INFINITY, sum = 0.f;
    __device__ __forceinline__ void add(float x) {
        if (x > m) { sum *= expf(m - x); m = x; }
        if (m > -INFINITY) sum += expf(x - m);
    }
    __device__ __forceinline__ void add4(float a, float b, float c, float d) {
        const float mx = fmaxf(fmaxf(a, b), fmaxf(c, d));
        if (mx > m) { sum *= expf(m - mx); m = mx; }              // expf(-inf) = 0 on the first group
        if (m > -INFINITY) sum += expf(a - m) + expf(b - m) + expf(c - m) + expf(d - m);
    }
    __device__ __forceinline__ void merge(float om, float os) {
        const float mx = fmaxf(m, om);
        if (mx == -INFINITY) return;                               // both empty
        sum = sum * expf(m - mx) + os * expf(om - mx);
        m = mx;
    }
    // across the 64 lanes of a wave, in a fixed order: every lane ends with the wave's pair
    __device__ __forceinline__ void wave_merge() {
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(m, o, 64), os = __shfl_xor(sum, o, 64);
            merge(om, os);
        }
    }
};

// ---- sorted register list -------------------------------------------------------------------------------------------------------------
// A thread's K best (value, index), best first, in registers: every index below is static.  Empty entries are (-inf, SEL_NONE).
template <int K>
struct SortedList {
    float v[K];
    int i[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < K; k++) { v[k] = -INFINITY; i[k] = SEL_NONE; }
    }
    // enter by one compare against the last entry, sink with static-index swaps
    __device__ __forceinline__ void enter(float val, int idx) {
        if (cand_better(val, idx, v[K - 1], i[K - 1])) {
            v[K - 1] = val; i[K - 1] = idx;
#pragma unroll
            for (int k = K - 1; k > 0; k--) {
                if (cand_better(v[k], i[k], v[k - 1], i[k - 1])) {
                    const float tv = v[k]; v[k] = v[k - 1]; v[k - 1] = tv;
                    const int ti = i[k]; i[k] = i[k - 1]; i[k - 1] = ti;
                }
            }
        }
    }
    // pop the head if it is the block's pick bi (indices are unique: exactly one owner)
    __device__ __forceinline__ void retire(int bi) {
        if (i[0] == bi && bi != SEL_NONE) {
#pragma unroll
            for (int q = 0; q + 1 < K; q++) { v[q] = v[q + 1]; i[q] = i[q + 1]; }
            v[K - 1] = -INFINITY; i[K - 1] = SEL_NONE;
        }
    }
};

// ---- block arg-max --------------------------------------------------------------------------------------------------------------------
// One round of block arg-max under cand_better, for blocks of NW full waves: wave arg-max by shuffles, the wave winners meet in LDS
// (red / redi hold 2 NW entries, double-buffered on k, so a round costs one barrier), every thread merges them.  On return every thread
// holds the block's best (bv, bi); no candidate left: bi = SEL_NONE.
template <int NW>
__device__ __forceinline__ void block_argmax(int k, float& bv, int& bi, float* red, int* redi) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (cand_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { red[(k & 1) * NW + wv] = bv; redi[(k & 1) * NW + wv] = bi; }
    __syncthreads();
    bv = red[(k & 1) * NW]; bi = redi[(k & 1) * NW];
#pragma unroll
    for (int w = 1; w < NW; w++) {
        const float ov = red[(k & 1) * NW + w];
        const int oi = redi[(k & 1) * NW + w];
        if (cand_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
}
// thread 0 records the round's result as pick k (no candidate left: -inf, SEL_NONE)
__device__ __forceinline__ void record_pick(int k, float bv, int bi, float* sel_v, int* sel_i) {
    if (threadIdx.x == 0) { sel_v[k] = bi != SEL_NONE ? bv : -INFINITY; sel_i[k] = bi; }
}

// The `n_pick` best of the n (value, flat index) candidates of an LDS list, best first, into sel_v / sel_i: one arg-max round per pick; the
// winner is retired by its flat index (unique: one owner; visible after the round's closing barrier).  Blocks of NT threads.
template <int NT>
__device__ __forceinline__ void pick_from_list(const float* cv, int* ci, int n, int n_pick, float* red, int* redi, float* sel_v, int* sel_i) {
    const int tid = threadIdx.x;
    for (int k = 0; k < n_pick; k++) {
        float bv = -INFINITY;
        int bi = SEL_NONE;
        for (int c = tid; c < n; c += NT)
            if (ci[c] != SEL_NONE && cand_better(cv[c], ci[c], bv, bi)) { bv = cv[c]; bi = ci[c]; }
        block_argmax<NT / 64>(k, bv, bi, red, redi);
        record_pick(k, bv, bi, sel_v, sel_i);
        for (int c = tid; c < n; c += NT)
            if (ci[c] == bi) ci[c] = SEL_NONE;
        __syncthreads();
    }
}

// The TB-th largest of the 256 threads' maxima: a lower bound of the block's TB-th best key (equal maxima leave together: the bound only
// gets lower, which is still valid).  red: 8 floats.
template <int TB>
__device__ __forceinline__ float kth_bound(float tmax, float* red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float thr = -INFINITY;
    for (int k = 0; k < TB; k++) {
        float bv = wave_max(tmax);
        if (lane == 0) red[(k & 1) * 4 + wv] = bv;
        __syncthreads();
        thr = fmaxf(fmaxf(red[(k & 1) * 4], red[(k & 1) * 4 + 1]), fmaxf(red[(k & 1) * 4 + 2], red[(k & 1) * 4 + 3]));
        if (tmax == thr) tmax = -INFINITY;
    }
    return thr;
}

}  // namespace CC_NS
