// Constrained decoding: token bans applied to one step's logits on the device, in front of the beam update (beam.hip) or the sampler
// (sample.hip).  A ban is "the logit is -inf before the softmax" (the convention of the reference's top_k_top_p_filtering, utils.py:5-30):
// the banned mass is renormalised over the allowed tokens.  Three rules make a row's banned set (include/clipcap_hip.h cc_logits_constrain):
// no-repeat n-grams over the row's token history, one host-chosen token (the stop token while a caption is shorter than min_length) and a
// fixed suppress list.  fp32 / integer work only, so this unit is built once (Makefile).
//
// Why this cannot be a masked_fill from outside: the fused beam update (k_beam_fused) never scans the logits — it bounds every 64-column
// block by the lm_head epilogue's partial (pmax, psum) and takes the TB-th largest bound as a LOWER bound of the TB-th best candidate.  A
// banned token that is its block's maximum would leave that bound too high (fewer than `beam` real candidates survive) and every banned
// token leaves its block's psum, hence the row's softmax denominator, too large.  So the partials of exactly the touched blocks are
// rebuilt here, in the same launch.
#include "layout.h"

using namespace CC_NS;

namespace {

constexpr int CN_T = 256;                 // threads per row (4 waves)
constexpr int CN_HIST_MAX = 1024;         // history tokens per row (GPT-2's n_positions)
constexpr int CN_SUPPRESS_MAX = 1023;
constexpr int CN_WORDS = 1024;            // touched-block bitmap: 32 blocks of 64 columns per word
constexpr int CN_VMAX = CN_WORDS * 32 * 64;

// One workgroup owns one row from start to end; nothing is exchanged between workgroups.
//   1. the row's history goes to LDS as it is (int32 or int64 elements), the touched-block bitmap is cleared
//   2. every thread finds bans (one history position per thread does the suffix compare; the suppress list is strided over the block;
//      thread 0 adds ban_token), stores -inf and marks the token's 64-column block.  Several threads may ban the same token or mark the
//      same block: all of them store the same value / set the same bit, so the outcome does not depend on who found what.
//   3. barrier (the -inf stores are visible to the whole workgroup after it)
//   4. the waves share the bitmap's words; for every marked block a wave re-reads the block's real columns (v < V) and rewrites its
//      pmax / psum.  A block is rebuilt once however many bans fell into it; a block left without a finite entry gets (-inf, 0), which the
//      beam update treats as empty.
// Untouched blocks, the padding columns [V, ldl) and skipped rows are never written.
template <class HT>
__global__ __launch_bounds__(CN_T) void k_logits_constrain(float* logits, size_t ldl, int V, float* pmax, float* psum, int npart, const HT* __restrict__ hist,
                                                           size_t hist_stride, int n, int g, int ban_token, const int* __restrict__ suppress,
                                                           int n_suppress, const unsigned char* __restrict__ skip) {
    __shared__ HT h[CN_HIST_MAX];                                       // raw ids: the suffix compare sees what the caller wrote
    __shared__ unsigned touched[CN_WORDS];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (skip && skip[row]) return;                                      // block-uniform, before any barrier
    float* lg = logits + (size_t)row * ldl;
    const int nblk = (V + 63) >> 6, nwords = (nblk + 31) >> 5;
    const bool repair = pmax != nullptr;
    const bool ngram = g > 0 && n >= g;
    if (ngram)
        for (int i = tid; i < n; i += CN_T) h[i] = hist[(size_t)row * hist_stride + i];
    if (repair)
        for (int w = tid; w < nwords; w += CN_T) touched[w] = 0u;
    __syncthreads();
    auto ban = [&](long long t) {
        if (t < 0 || t >= V) return;                                    // ids outside the vocabulary ban nothing (and write nothing)
        lg[t] = -INFINITY;
        if (repair) atomicOr(&touched[(int)t >> 11], 1u << (((int)t >> 6) & 31));
    };
    if (ngram) {
        // h[i : i+g-1] == h[n-g+1 : n]  ->  ban h[i+g-1], for i in [0, n-g] (g == 1: the empty prefix matches everywhere)
        for (int i = tid; i <= n - g; i += CN_T) {
            bool same = true;
            for (int k = 0; k < g - 1; k++) same = same && h[i + k] == h[n - g + 1 + k];
            if (same) ban(h[i + g - 1]);
        }
    }
    for (int i = tid; i < n_suppress; i += CN_T) ban(suppress[i]);
    if (tid == 0) ban(ban_token);
    if (!repair) return;
    __syncthreads();
    for (int w = wv; w < nwords; w += CN_T / 64) {
        unsigned bits = touched[w];                                     // wave-uniform: the whole wave takes every reduction below
        while (bits) {
            const int j = w * 32 + (__ffs(bits) - 1);
            bits &= bits - 1;
            const int v = j * 64 + lane;
            const float x = v < V ? lg[v] : -INFINITY;
            const float m = wave_max(x);
            const float s = wave_sum(x > -INFINITY ? expf(x - m) : 0.f);
            if (lane == 0) {
                pmax[(size_t)row * npart + j] = m;
                psum[(size_t)row * npart + j] = s;
            }
        }
    }
}

}  // namespace

extern "C" {

int CC_API(cc_logits_constrain)(float* logits, int32_t R, int32_t V, int64_t ldl, float* lpart, int32_t npart, const void* history,
                                int32_t hist_elem_bytes, int64_t hist_stride, int32_t hist_len, int32_t no_repeat_ngram, int32_t ban_token,
                                const int32_t* suppress, int32_t n_suppress, const uint8_t* skip_rows, void* stream) {
    if (!logits || R < 0 || V <= 0 || ldl < V || no_repeat_ngram < 0 || hist_len < 0 || n_suppress < 0 || ban_token < -1 || ban_token >= V ||
        (n_suppress > 0 && !suppress) || (lpart && (int64_t)npart * 64 < V))
        return CC_ERR_ARG;
    const bool use_hist = no_repeat_ngram > 0 && hist_len > 0;
    if (use_hist && (!history || (hist_elem_bytes != 4 && hist_elem_bytes != 8) || hist_stride < hist_len)) return CC_ERR_ARG;
    if (hist_len > CN_HIST_MAX || n_suppress > CN_SUPPRESS_MAX || V > CN_VMAX) return CC_ERR_SHAPE;
    if (R == 0 || (!(use_hist && hist_len >= no_repeat_ngram) && ban_token < 0 && n_suppress == 0)) return CC_OK;      // nothing can be banned
    float* pmax = lpart;
    float* psum = lpart ? lpart + (size_t)R * npart : nullptr;
    hipStream_t st = S_(stream);
    if (use_hist && hist_elem_bytes == 8)
        hipLaunchKernelGGL(k_logits_constrain<long long>, dim3(R), dim3(CN_T), 0, st, logits, (size_t)ldl, V, pmax, psum, npart,
                           static_cast<const long long*>(history), (size_t)hist_stride, hist_len, no_repeat_ngram, ban_token, suppress, n_suppress,
                           skip_rows);
    else
        hipLaunchKernelGGL(k_logits_constrain<int>, dim3(R), dim3(CN_T), 0, st, logits, (size_t)ldl, V, pmax, psum, npart,
                           static_cast<const int*>(use_hist ? history : nullptr), (size_t)hist_stride, use_hist ? hist_len : 0, no_repeat_ngram,
                           ban_token, suppress, n_suppress, skip_rows);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // extern "C"
