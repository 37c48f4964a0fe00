// Contrastive search (Su et al., 2022; not in the reference): the two device steps around the decode forward (include/clipcap_hip.h
// cc_contrastive_topk / cc_contrastive_select).  k_contrastive_topk turns one logits row per caption into its k candidates (ids and softmax
// probabilities); after the forward has run the candidates, k_contrastive_select takes every candidate's largest cosine similarity to the
// context's hidden states, scores, picks the winner and commits it (caption, history, flags, the rows cc_beam_advance and
// cc_logits_constrain need).  The unit vectors come from cc_decode_hidden_unit (decode.hip).  fp32 / integer work only, so this unit is
// built once (Makefile).  Plain C++: no inline assembly.
#include "layout.h"
#include "select.hip.h"

using namespace CC_NS;

namespace {

constexpr int CS_KMAX = 8;
constexpr int CS_VMAX = 2097152;
constexpr int CS_DMAX = 2048;
constexpr int TK_T = 512;                 // threads per caption in the top-k kernel (8 waves)
constexpr int SL_T = 256;                 // threads per caption in the select kernel (4 waves)

// ---- top-k with probabilities ------------------------------------------------------------------------------------------------------------
// One workgroup per caption, the row read once.  Every thread keeps, over its share of the row, a running softmax pair and its own K best
// (value, id) in a sorted register list (select.hip.h, as k_beam_rowstats and the beam kernels' overflow path do).  The block then takes K
// rounds of arg-max over the threads' list heads; the winner's owner pops its list.  The block's K best are among the threads' K best, so
// nothing is missed.  -inf never enters a list: an empty head is (-inf, SEL_NONE).
template <int K, bool VEC>   // VEC: rows are 16-B aligned (ldl % 4 == 0, aligned base) -> float4 loads
__global__ __launch_bounds__(TK_T) void k_contrastive_topk(const float* __restrict__ logits, size_t ldl, int rows_per, const int* __restrict__ sel,
                                                           int V, const unsigned char* __restrict__ stopped, int* __restrict__ cand_tok,
                                                           float* __restrict__ cand_prob) {
    constexpr int NW = TK_T / 64;
    __shared__ float redm[NW], reds[NW], redv[2 * NW];
    __shared__ int redi[2 * NW];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (stopped && stopped[s]) {                                        // block-uniform, before any barrier; the row is not read
        if (tid < K) { cand_tok[s * K + tid] = 0; cand_prob[s * K + tid] = -1.0f; }
        return;
    }
    const float* lg = logits + ((size_t)s * rows_per + (sel ? min(max(sel[s], 0), rows_per - 1) : 0)) * ldl;   // never outside the caption's rows
    SortedList<K> top;
    top.clear();
    SoftmaxPair p;
    auto take = [&](float x, int v) {
        if (x > -INFINITY) top.enter(x, v);
    };
    const int V4 = VEC ? (V >> 2) : 0;
    for (int v = tid; v < V4; v += TK_T) {
        const float4 x = reinterpret_cast<const float4*>(lg)[v];
        p.add4(x.x, x.y, x.z, x.w);
        take(x.x, 4 * v); take(x.y, 4 * v + 1); take(x.z, 4 * v + 2); take(x.w, 4 * v + 3);
    }
    for (int v = V4 * 4 + tid; v < V; v += TK_T) {
        const float x = lg[v];
        p.add(x);
        take(x, v);
    }
    // the row's (max, sum): pairs merged across lanes and waves in a fixed order
    p.wave_merge();
    if (lane == 0) { redm[wv] = p.m; reds[wv] = p.sum; }
    __syncthreads();
    p.m = redm[0]; p.sum = reds[0];
    for (int i = 1; i < NW; i++) p.merge(redm[i], reds[i]);             // every thread, the same order: block-uniform (m, sum)
    // K rounds of block arg-max over the list heads
#pragma unroll
    for (int r = 0; r < K; r++) {
        float bv = top.v[0];
        int bi = top.i[0];
        block_argmax<NW>(r, bv, bi, redv, redi);
        top.retire(bi);
        if (tid == 0) {
            const bool ok = bi != SEL_NONE;
            cand_tok[s * K + r] = ok ? bi : 0;
            cand_prob[s * K + r] = ok ? expf(bv - p.m) / p.sum : -1.0f;
        }
    }
}

// ---- similarity, max, score, select, commit -------------------------------------------------------------------------------------------------
// One workgroup of 4 waves per caption.  Dynamic LDS: the K candidate vectors, K * D floats (64 KB at K = 8, D = 2048).
//   1. the candidates go to LDS (16-B loads and stores)
//   2. wave w walks history positions hist_lo + w, + 4, ...: a row is read once (16 B per lane per trip), multiplied into all K candidates,
//      the K partial sums reduced over the lanes (wave_sum: DPP, a fixed order), each wave keeps its K running maxima
//   3. barrier; the waves' maxima meet in the front of the LDS buffer (the candidates there are not read again: the commit copies the
//      winner from global memory); barrier
//   4. thread 0 merges the maxima (a maximum does not depend on the order), scores the valid slots in slot order and commits the scalars;
//      barrier; the workgroup copies the winner's vector into hist[s][hist_n] and writes the K src_rows / skip_rows
// A caption that had stopped leaves at the top (block-uniform: every thread reads the flag before thread 0 can write it, which happens
// after two barriers).
template <int K>
__global__ __launch_bounds__(SL_T) void k_contrastive_select(int D, const float* __restrict__ cand_h, const float* __restrict__ cand_prob,
                                                             const int* __restrict__ cand_tok, float* hist, int hist_ld, int hist_lo, int hist_n,
                                                             float alpha, int stop_token, unsigned char* stopped, int* lengths, int* sel,
                                                             int* src_rows, unsigned char* skip_rows, int* captions, int cap_ld, int step,
                                                             float* sel_score) {
    extern __shared__ __attribute__((aligned(16))) float4 cs_cand[];    // [K][D / 4]
    constexpr int NW = SL_T / 64;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (stopped[s]) {
        if (tid == 0) {
            sel[s] = 0;
            captions[(size_t)s * cap_ld + step] = 0;
            if (sel_score) sel_score[s] = 0.f;
        }
        if (tid < K) { src_rows[s * K + tid] = 0; skip_rows[s * K + tid] = 1; }
        return;
    }
    const int D4 = D >> 2;
    const float4* ch = reinterpret_cast<const float4*>(cand_h + (size_t)s * K * D);
    for (int i = tid; i < K * D4; i += SL_T) cs_cand[i] = ch[i];
    __syncthreads();
    float mx[K];
#pragma unroll
    for (int c = 0; c < K; c++) mx[c] = -INFINITY;
    for (int j = hist_lo + wv; j < hist_n; j += NW) {                   // wave-uniform bounds: the whole wave takes every reduction
        const float4* hr = reinterpret_cast<const float4*>(hist + ((size_t)s * hist_ld + j) * D);
        float acc[K];
#pragma unroll
        for (int c = 0; c < K; c++) acc[c] = 0.f;
        for (int i = lane; i < D4; i += 64) {
            const float4 h = hr[i];
#pragma unroll
            for (int c = 0; c < K; c++) {
                const float4 v = cs_cand[c * D4 + i];
                acc[c] += (h.x * v.x + h.y * v.y) + (h.z * v.z + h.w * v.w);
            }
        }
#pragma unroll
        for (int c = 0; c < K; c++) mx[c] = fmaxf(mx[c], wave_sum(acc[c]));
    }
    __syncthreads();
    float* red = reinterpret_cast<float*>(cs_cand);                     // [NW][8] maxima, then one int: the winner
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < K; c++) red[wv * CS_KMAX + c] = mx[c];
    }
    __syncthreads();
    int* wsh = reinterpret_cast<int*>(red + NW * CS_KMAX);
    if (tid == 0) {
        int w = -1;
        float best = 0.f;
#pragma unroll
        for (int c = 0; c < K; c++) {
            float deg = red[c];
#pragma unroll
            for (int x = 1; x < NW; x++) deg = fmaxf(deg, red[x * CS_KMAX + c]);
            if (hist_n <= hist_lo) deg = 0.f;
            const float p = cand_prob[s * K + c];
            const float sc = (1.0f - alpha) * p - alpha * deg;
            if (p >= 0.f && (w < 0 || sc > best)) { w = c; best = sc; }
        }
        const int token = w >= 0 ? cand_tok[s * K + w] : stop_token;
        sel[s] = w >= 0 ? w : 0;
        captions[(size_t)s * cap_ld + step] = token;
        lengths[s] += 1;
        stopped[s] = token == stop_token ? 1 : 0;
        if (sel_score) sel_score[s] = w >= 0 ? best : 0.f;
        wsh[0] = w;
        wsh[1] = token == stop_token ? 1 : 0;
    }
    __syncthreads();
    const int w = wsh[0], st = wsh[1];
    if (tid < K) { src_rows[s * K + tid] = w >= 0 ? w : 0; skip_rows[s * K + tid] = (tid != w || st) ? 1 : 0; }
    if (w >= 0) {
        float4* dst = reinterpret_cast<float4*>(hist + ((size_t)s * hist_ld + hist_n) * D);
        for (int i = tid; i < D4; i += SL_T) dst[i] = ch[w * D4 + i];
    }
}

}  // namespace

extern "C" {

int CC_API(cc_contrastive_topk)(const float* logits, int64_t ldl, int32_t S, int32_t rows_per, const int32_t* sel, int32_t V, int32_t k,
                                const uint8_t* stopped, int32_t* cand_tok, float* cand_prob, void* stream) {
    if (!logits || !cand_tok || !cand_prob || S < 0 || rows_per < 1 || k < 1 || k > CS_KMAX || V < 1 || ldl < V) return CC_ERR_ARG;
    if (V > CS_VMAX) return CC_ERR_SHAPE;
    if (S == 0) return CC_OK;
    hipStream_t st = S_(stream);
    const bool vec = (ldl & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
#define CC_TK(K_)                                                                                                                                  \
    case K_:                                                                                                                                       \
        if (vec) hipLaunchKernelGGL((k_contrastive_topk<K_, true>), dim3(S), dim3(TK_T), 0, st, logits, (size_t)ldl, rows_per, sel, V, stopped, cand_tok, cand_prob); \
        else hipLaunchKernelGGL((k_contrastive_topk<K_, false>), dim3(S), dim3(TK_T), 0, st, logits, (size_t)ldl, rows_per, sel, V, stopped, cand_tok, cand_prob);   \
        break;
    switch (k) { CC_TK(1) CC_TK(2) CC_TK(3) CC_TK(4) CC_TK(5) CC_TK(6) CC_TK(7) CC_TK(8) default: return CC_ERR_ARG; }
#undef CC_TK
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int CC_API(cc_contrastive_select)(int32_t S, int32_t k, int32_t D, const float* cand_h, const float* cand_prob, const int32_t* cand_tok, float* hist,
                                  int32_t hist_ld, int32_t hist_lo, int32_t hist_n, float alpha, int32_t stop_token, uint8_t* stopped, int32_t* lengths,
                                  int32_t* sel, int32_t* src_rows, uint8_t* skip_rows, int32_t* captions, int32_t cap_ld, int32_t step, float* sel_score,
                                  void* stream) {
    if (!cand_h || !cand_prob || !cand_tok || !hist || !stopped || !lengths || !sel || !src_rows || !skip_rows || !captions) return CC_ERR_ARG;
    if (S < 0 || k < 1 || k > CS_KMAX || D < 4 || hist_lo < 0 || hist_lo > hist_n || hist_n >= hist_ld || !(alpha >= 0.f && alpha <= 1.f) || step < 0 ||
        step >= cap_ld)
        return CC_ERR_ARG;                                              // (a NaN alpha fails both comparisons)
    if ((D & 3) || D > CS_DMAX) return CC_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(cand_h) & 15) || (reinterpret_cast<uintptr_t>(hist) & 15)) return CC_ERR_ARG;      // 16-byte loads and stores
    if (S == 0) return CC_OK;
    hipStream_t st = S_(stream);
    const size_t shm = std::max<size_t>((size_t)k * D * sizeof(float), (SL_T / 64 * CS_KMAX + 4) * sizeof(float));       // <= 64 KB
#define CC_SL(K_)                                                                                                                              \
    case K_:                                                                                                                                   \
        hipLaunchKernelGGL((k_contrastive_select<K_>), dim3(S), dim3(SL_T), shm, st, D, cand_h, cand_prob, cand_tok, hist, hist_ld, hist_lo, hist_n, \
                           alpha, stop_token, stopped, lengths, sel, src_rows, skip_rows, captions, cap_ld, step, sel_score);                \
        break;
    switch (k) { CC_SL(1) CC_SL(2) CC_SL(3) CC_SL(4) CC_SL(5) CC_SL(6) CC_SL(7) CC_SL(8) default: return CC_ERR_ARG; }
#undef CC_SL
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // extern "C"
