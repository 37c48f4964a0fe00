// What the beam updates share (beam.hip: cc_beam_step, cc_beam_group_step; lexbeam.hip: cc_beam_lex_step): the row statistics kernel, a
// candidate's value in the reference's arithmetic and the state update of one output slot.  One definition each, so the updates agree bit for bit.
#pragma once
#include "layout.h"
#include "select.hip.h"

namespace CC_NS {
namespace {

template <bool VEC>   // VEC: rows are 16-B aligned (ldl % 4 == 0, aligned base) -> float4 loads
__global__ __launch_bounds__(512) void k_beam_rowstats(const float* __restrict__ logits, size_t ldl, int V, float inv_temp, float* __restrict__ rs) {
    // one pass: every thread keeps a running (max, sum of exp(x - max)) pair, rescaling the sum when its max moves; pairs are merged
    // the same way across lanes and waves (the logits matrix, 64 MB at 320 x 50257, is read once instead of twice).
    // This is SoftmaxPair (select.hip.h) written out, and it stays written out: through the struct, or through free functions on
    // (m, sum) references, the kernel compiles to 73 / 80 more instructions with branches around expf where these lambdas give
    // selects (profiles/r19_a_select_refactor.md), and it reads every logit of every three-kernel update.  A change to the -inf guards
    // or the merge order is made in SoftmaxPair AND here.
    __shared__ float redm[8], reds[8];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* lg = logits + (size_t)row * ldl;
    const int V4 = VEC ? (V >> 2) : 0;
    float m = -INFINITY, sum = 0.f;
    auto add4 = [&](float a, float b, float c, float d) {
        const float mx = fmaxf(fmaxf(a, b), fmaxf(c, d));
        if (mx > m) { sum *= expf(m - mx); m = mx; }              // expf(-inf) = 0 on the first group
        if (m > -INFINITY) sum += expf(a - m) + expf(b - m) + expf(c - m) + expf(d - m);   // banned tokens (-inf, constrain.hip) first: no -inf - -inf
    };
    for (int v = tid; v < V4; v += 512) {
        const float4 x = reinterpret_cast<const float4*>(lg)[v];
        add4(x.x * inv_temp, x.y * inv_temp, x.z * inv_temp, x.w * inv_temp);
    }
    for (int v = V4 * 4 + tid; v < V; v += 512) {
        const float x = lg[v] * inv_temp;
        if (x > m) { sum *= expf(m - x); m = x; }
        if (m > -INFINITY) sum += expf(x - m);
    }
    auto merge = [&](float om, float os) {
        const float mx = fmaxf(m, om);
        if (mx == -INFINITY) return;                               // both empty
        sum = sum * expf(m - mx) + os * expf(om - mx);
        m = mx;
    };
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64), os = __shfl_xor(sum, o, 64);
        merge(om, os);
    }
    if ((tid & 63) == 0) { redm[tid >> 6] = m; reds[tid >> 6] = sum; }
    __syncthreads();
    if (tid == 0) {
        m = redm[0]; sum = reds[0];
        for (int i = 1; i < 8; i++) merge(redm[i], reds[i]);
        rs[2 * row] = m;
        rs[2 * row + 1] = sum;
    }
}

// What a candidate's value needs of its beam row: the stop flag, max and sum(exp) of the row's logits (over the temperature), log(sum),
// the beam's score so far and the length the candidate would have (seq_len + 1; a stopped beam keeps its length).  First step: sc = 0,
// len = 1, nothing stopped.
struct BeamRow {
    int st;
    float m, sum, lsum, sc, len;
};
// base.py:96-101: only token 0 continues a stopped beam, at the beam's own average
__device__ __forceinline__ float beam_stopped(const BeamRow& g, int v, int first) { return v == 0 ? (first ? 0.f : (g.sc + 0.f) / g.len) : -INFINITY; }
// DIV = true: the Hamming penalty of diverse beam search, c = picks of token v by the earlier beam groups.  c == 0 applies no operation at
// all, so one beam group is bit-identical to the plain update; DIV = false compiles neither the count nor the penalty.
// Cheap image of a candidate's value, monotone in the logit: exact for stopped beams, within ~1e-6 of beam_val otherwise
// (x t - m - log(sum) instead of log(exp(x t - m) / sum)).
template <bool DIV>
__device__ __forceinline__ float beam_key(const BeamRow& g, int v, float xraw, float inv_temp, int first, int c, float penalty) {
    if (g.st) return beam_stopped(g, v, first);
    float d = (xraw * inv_temp - g.m) - g.lsum;
    if constexpr (DIV) {
        if (c > 0) d -= penalty * (float)c;
    }
    return first ? d : (g.sc + d) * (1.0f / g.len);
}
// The candidate's value in the reference's arithmetic: softmax().log(), then the length-normalised sum (base.py:99-101)
template <bool DIV>
__device__ __forceinline__ float beam_val(const BeamRow& g, int v, float xraw, float inv_temp, int first, int c, float penalty) {
    if (g.st) return beam_stopped(g, v, first);
    float lp = logf(expf(xraw * inv_temp - g.m) / g.sum);
    if constexpr (DIV) {
        if (c > 0) lp -= penalty * (float)c;
    }
    return first ? lp : (g.sc + lp) / g.len;
}

// State update of base.py:86-119 for output slot o: the pick (val, token v) continues a source beam of length len (as BeamRow::len) and
// stop flag st; both are read by the caller before any slot is written.  scores = scores_sum_average * seq_lengths (base.py:114).
__device__ __forceinline__ void beam_commit(int o, float val, int b, int v, int first, int stop_token, float len, int st, float* scores,
                                            float* seq_len, unsigned char* stopped, int* next_tok, int* src_row) {
    float nl, nsc;
    int hs;
    if (first) { nl = 1.f; nsc = val; hs = 0; }
    else { nl = len; nsc = val * nl; hs = st; }
    hs |= (v == stop_token) ? 1 : 0;
    next_tok[o] = v;
    src_row[o] = b;
    scores[o] = nsc;
    seq_len[o] = nl;
    stopped[o] = (unsigned char)hs;
}

inline void launch_rowstats(hipStream_t st, const float* logits, int64_t ldl, int rows, int V, float inv_temp, float* rs) {
    if ((ldl & 3) || ((uintptr_t)logits & 15))
        hipLaunchKernelGGL(k_beam_rowstats<false>, dim3(rows), dim3(512), 0, st, logits, (size_t)ldl, V, inv_temp, rs);
    else
        hipLaunchKernelGGL(k_beam_rowstats<true>, dim3(rows), dim3(512), 0, st, logits, (size_t)ldl, V, inv_temp, rs);
}

}  // namespace
}  // namespace CC_NS
