// Lexically constrained beam search with dynamic beam allocation (Post & Vilar, NAACL 2018; the constraint idea: Anderson et al., EMNLP
// 2017; not in the reference): the device update that makes a beam produce required phrases (include/clipcap_hip.h cc_beam_lex_step).
// Every beam row carries which phrases it has produced and how far it is into one (lex_state.h), a hypothesis may stop only with every
// phrase produced, and the fixed `beam` slots of a sample are divided between its candidates by how many constraint tokens they have met.
// Three launches, stream-ordered, no atomics:
//   k_beam_rowstats : beam.hip.h, as cc_beam_step: max and sum(exp) of every row
//   k_lex_rows      : one block per live parent row: the row's `beam` best valid (value, token) by beam_val, in per-thread sorted lists
//                     merged by block arg-max rounds, plus a direct gather of the at most n_phr + 1 tokens that advance the row's phrases
//   k_lex_final     : one 64-thread block per sample over at most beam * (beam + n_phr + 1) candidates: the candidate set, the
//                     transition, the banks, the round-robin (as two counting ranks) and the commit, in LDS
// Values are cc_beam_step's (beam_val on the statistics of k_beam_rowstats), so without phrases the result is cc_beam_step's bit for bit.
// fp32 / integer work only: built once (Makefile).  Plain C++: no inline assembly.
#include "beam.hip.h"
#include "lex_state.h"

using namespace CC_NS;

namespace {

constexpr int LX_MAX = 16;                // widest beam
constexpr int LX_VMAX = 2097152;          // 16 * 2^21 flat indices stay far inside int
constexpr int LR_T = 512;                 // threads per parent row (8 waves), as k_beam_rowstats and k_gumbel_rows
constexpr int LX_TAB = LEX_MAX_PHR * LEX_MAX_LEN;
constexpr int LX_CW_MAX = LX_MAX + LEX_MAX_PHR + 1;      // kept candidates per parent row
constexpr int LX_CAND = LX_MAX * LX_CW_MAX;              // 400 per sample

// Workspace: row statistics [S * beam][2] | per row: list values [beam], list tokens [beam], phrase-token values [n_phr + 1], phrase tokens
// [n_phr + 1] (4-byte words)
__host__ __device__ __forceinline__ int lx_cw(int beam, int n_phr) { return beam + n_phr + 1; }
__host__ __device__ __forceinline__ size_t lx_row_words(int beam, int n_phr) { return 2 * (size_t)lx_cw(beam, n_phr); }

// the parent row's record (first: the sample's row 0 with no history)
__device__ __forceinline__ BeamRow lx_row(int row, int first, const float* rs, const float* scores, const float* seq_len, const unsigned char* stopped) {
    BeamRow g;
    g.st = !first && stopped[row];
    g.m = rs[2 * row]; g.sum = rs[2 * row + 1];
    g.lsum = logf(g.sum);
    g.sc = first ? 0.f : scores[row];
    g.len = first ? 1.f : (seq_len[row] + (g.st ? 0.f : 1.f));
    return g;
}

// K: length of the register lists (>= beam; 16 serves every width without a compile-time list of its own).  VEC: rows are 16-B aligned.
template <int K, bool VEC>
__global__ __launch_bounds__(LR_T) void k_lex_rows(const float* __restrict__ logits, size_t ldl, int beam, int V, float inv_temp, int first,
                                                   int stop_token, const int* __restrict__ phrases, int n_phr, int phr_len,
                                                   const float* __restrict__ rs, const float* __restrict__ scores,
                                                   const float* __restrict__ seq_len, const unsigned char* __restrict__ stopped,
                                                   const int* __restrict__ lex_state, float* __restrict__ rows_ws) {
    constexpr int NW = LR_T / 64;
    __shared__ float redv[2 * NW];
    __shared__ int redi[2 * NW];
    __shared__ float sel_v[LX_MAX];
    __shared__ int sel_t[LX_MAX];
    const int tid = threadIdx.x;
    const int row = first ? blockIdx.x * beam : blockIdx.x;             // the first step reads row 0 of every sample
    if (!first && stopped[row]) return;                                 // block-uniform, before any barrier; the row is not read
    const int s = row / beam;
    const float* lg = logits + (size_t)row * ldl;
    const int* tab = phrases + (size_t)s * n_phr * phr_len;             // not followed when n_phr == 0
    const BeamRow g = lx_row(row, first, rs, scores, seq_len, stopped);
    const int state = first ? 0 : lex_state[row];
    const bool may_stop = lex_met(state) == lex_full(tab, n_phr, phr_len);
    // a valid candidate's value, or -inf: the stop token is no candidate before every phrase has been produced (the softmax keeps it)
    auto value = [&](int v, float xraw) -> float {
        if (v == stop_token && !may_stop) return -INFINITY;
        const float val = beam_val<false>(g, v, xraw, inv_temp, first, 0, 0.f);
        return val > -INFINITY ? val : -INFINITY;                       // NaN is no candidate either
    };
    SortedList<K> top;
    top.clear();
    // the exact value (expf, divide, logf) only for a token whose cheap key could still enter the list (within ~1e-6 of it; margin 1e-3)
    auto take = [&](float xraw, int v) {
        if (beam_key<false>(g, v, xraw, inv_temp, first, 0, 0.f) + 1e-3f < top.v[K - 1]) return;
        const float val = value(v, xraw);
        if (val > -INFINITY) top.enter(val, v);
    };
    const int NG = (V + 3) >> 2;
    for (int q = tid; q < NG; q += LR_T) {
        if (VEC && 4 * q + 3 < V) {
            const float4 x = reinterpret_cast<const float4*>(lg)[q];
            take(x.x, 4 * q); take(x.y, 4 * q + 1); take(x.z, 4 * q + 2); take(x.w, 4 * q + 3);
        } else {                                                        // unaligned rows, and the last group of a row whose V is no multiple of 4
            for (int k = 0; k < 4; k++)
                if (4 * q + k < V) take(lg[4 * q + k], 4 * q + k);
        }
    }
    // `beam` rounds of block arg-max over the list heads (value descending, token ascending); the winner's owner pops its list
    for (int r = 0; r < beam; r++) {
        float bv = top.v[0];
        int bi = top.i[0];
        block_argmax<NW>(r, bv, bi, redv, redi);
        top.retire(bi);
        if (tid == 0) { sel_v[r] = bi != SEL_NONE ? bv : -INFINITY; sel_t[r] = bi; }
    }
    __syncthreads();
    const int cw = lx_cw(beam, n_phr);
    float* out = rows_ws + (size_t)row * lx_row_words(beam, n_phr);
    int* outi = reinterpret_cast<int*>(out);
    if (tid < beam) {                                                   // every entry is written: the kept tokens, best first
        out[tid] = sel_v[tid];
        outi[cw + tid] = sel_t[tid];
    }
    // the tokens that advance the row's phrases: entry 0 the next token of the phrase in progress, entry c + 1 the first token of unmet phrase c
    if (tid >= 64 && tid < 64 + n_phr + 1) {
        const int j = tid - 64;
        int v = -1;
        if (j == 0) {
            const int cur = lex_cur(state), pos = lex_pos(state);
            if (cur >= 0 && cur < n_phr && pos < phr_len) v = tab[cur * phr_len + pos];
        } else if (!(lex_met(state) >> (j - 1) & 1)) {
            v = tab[(j - 1) * phr_len];
        }
        float val = -INFINITY;
        if (v >= 0 && v < V) val = value(v, lg[v]);                      // an id outside [0, V) never matches
        out[beam + j] = val;
        outi[cw + beam + j] = val > -INFINITY ? v : SEL_NONE;
    }
}

__global__ __launch_bounds__(64) void k_lex_final(int beam, int V, int first, int stop_token, const int* __restrict__ phrases, int n_phr, int phr_len,
                                                  const float* __restrict__ rows_ws, float* __restrict__ scores, float* __restrict__ seq_len,
                                                  unsigned char* __restrict__ stopped, int* __restrict__ lex_state, int* __restrict__ next_tok,
                                                  int* __restrict__ src_row) {
    __shared__ float red[2];
    __shared__ int redi[2];
    __shared__ int s_tab[LX_TAB];
    __shared__ float s_len[LX_MAX], s_avg[LX_MAX];
    __shared__ int s_st[LX_MAX], s_state[LX_MAX];
    __shared__ float cval[LX_CAND];
    __shared__ int cflat[LX_CAND], ctop[LX_CAND], cnew[LX_CAND], cbank[LX_CAND], crank[LX_CAND];
    __shared__ float sel_v[LX_MAX];
    __shared__ int sel_i[LX_MAX], slot[LX_MAX];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int nrows = first ? 1 : beam;
    const int cw = lx_cw(beam, n_phr), ncand = nrows * cw;
    const int ntab = n_phr * phr_len;
    // the sample's phrases and the parents' state, read before any slot is written; a stopped parent's workspace row is not read
    for (int i = tid; i < ntab; i += 64) s_tab[i] = phrases[(size_t)s * ntab + i];
    if (tid < beam) {
        const int r = s * beam + tid;
        const int st = first ? 0 : stopped[r];
        s_st[tid] = st;
        s_len[tid] = first ? 1.f : seq_len[r] + (st ? 0.f : 1.f);       // BeamRow::len
        BeamRow g;
        g.st = st; g.m = 0.f; g.sum = 1.f; g.lsum = 0.f;
        g.sc = first ? 0.f : scores[r]; g.len = s_len[tid];
        s_avg[tid] = beam_stopped(g, 0, first);                          // a stopped parent's single continuation: token 0 at its own average
        s_state[tid] = first ? 0 : lex_state[r];
        slot[tid] = -1;
    }
    __syncthreads();
    // 1. the kept candidates of every parent: entries [0, beam) of a row are its list (best first), the rest its phrase tokens
    for (int c = tid; c < ncand; c += 64) {
        const int b = c / cw, j = c - b * cw;
        float val = -INFINITY;
        int flat = SEL_NONE;
        if (s_st[b]) {
            if (j == 0 && s_avg[b] > -INFINITY) { val = s_avg[b]; flat = b * V; }    // an empty slot (-inf) is no candidate: it stays empty
        } else {
            const float* rw = rows_ws + (size_t)(s * beam + b) * lx_row_words(beam, n_phr);
            const float x = rw[j];
            const int v = reinterpret_cast<const int*>(rw)[cw + j];
            if (v != SEL_NONE && x > -INFINITY) { val = x; flat = b * V + min(max(v, 0), V - 1); }   // written by k_lex_rows: in [0, V)
        }
        cval[c] = val;
        cflat[c] = flat;
        ctop[c] = j < beam ? flat : SEL_NONE;
    }
    __syncthreads();
    // 2. T: the `beam` best valid candidates of the sample are among the rows' lists
    pick_from_list<64>(cval, ctop, ncand, beam, red, redi, sel_v, sel_i);
    // 3. membership of K = T + every row's best (B) + the phrase tokens (P), one entry per flat index: a phrase token that a list entry of its
    //    row also holds keeps that entry and drops out itself; cnew = the state after the candidate, cbank = its tokens_met
    for (int c = tid; c < ncand; c += 64) {
        const int b = c / cw, j = c - b * cw, flat = cflat[c];
        bool in = flat != SEL_NONE;
        if (in && j < beam) {
            in = j == 0;
            for (int k = 0; k < beam; k++) in = in || sel_i[k] == flat;
            for (int q = beam; q < cw; q++) in = in || cflat[b * cw + q] == flat;
        } else if (in) {
            for (int q = 0; q < j; q++) in = in && cflat[b * cw + q] != flat;
        }
        int st = 0, bank = -1;
        if (in) {
            st = s_st[b] ? s_state[b] : lex_next(s_state[b], flat - b * V, s_tab, n_phr, phr_len);
            bank = lex_tokens_met(st, s_tab, n_phr, phr_len);
        }
        cnew[c] = st;
        cbank[c] = bank;                                                 // -1: not in K
    }
    __syncthreads();
    // 4. the round-robin over the banks, highest first, each giving its best untaken candidate per round: the order is (rank inside the bank
    //    ascending, bank descending), so a candidate's slot is a count of the members before it
    for (int c = tid; c < ncand; c += 64) {
        int r = 0;
        if (cbank[c] >= 0)
            for (int q = 0; q < ncand; q++) r += (cbank[q] == cbank[c] && cand_better(cval[q], cflat[q], cval[c], cflat[c])) ? 1 : 0;
        crank[c] = r;
    }
    __syncthreads();
    for (int c = tid; c < ncand; c += 64) {
        if (cbank[c] < 0) continue;
        int p = 0;
        for (int q = 0; q < ncand; q++)
            p += (cbank[q] >= 0 && (crank[q] < crank[c] || (crank[q] == crank[c] && cbank[q] > cbank[c]))) ? 1 : 0;
        if (p < beam) slot[p] = c;                                       // positions are unique: one writer per slot
    }
    __syncthreads();
    // 5. the commit, slots in picking order
    if (tid < beam) {
        const int o = s * beam + tid, c = slot[tid];
        if (c < 0) {                                                     // fewer candidates than slots: an empty slot, which stays empty
            next_tok[o] = 0;
            src_row[o] = 0;
            scores[o] = -INFINITY;
            seq_len[o] = first ? 1.f : s_len[0] - (s_st[0] ? 0.f : 1.f);    // row 0's length as a stopped parent passes it on
            stopped[o] = 1;
            lex_state[o] = 0;
        } else {
            const int b = c / cw, v = cflat[c] - b * V;                  // b < nrows by construction
            beam_commit(o, cval[c], b, v, first, stop_token, s_len[b], s_st[b], scores, seq_len, stopped, next_tok, src_row);
            lex_state[o] = cnew[c];
        }
    }
}

template <int K>
void launch_lex_rows(hipStream_t st, int blocks, const float* logits, int64_t ldl, int beam, int V, float inv_temp, int first, int stop_token,
                     const int* phrases, int n_phr, int phr_len, const float* rs, const float* scores, const float* seq_len, const uint8_t* stopped,
                     const int* lex_state, float* rows_ws) {
    if ((ldl & 3) || ((uintptr_t)logits & 15))
        hipLaunchKernelGGL((k_lex_rows<K, false>), dim3(blocks), dim3(LR_T), 0, st, logits, (size_t)ldl, beam, V, inv_temp, first, stop_token, phrases,
                           n_phr, phr_len, rs, scores, seq_len, stopped, lex_state, rows_ws);
    else
        hipLaunchKernelGGL((k_lex_rows<K, true>), dim3(blocks), dim3(LR_T), 0, st, logits, (size_t)ldl, beam, V, inv_temp, first, stop_token, phrases,
                           n_phr, phr_len, rs, scores, seq_len, stopped, lex_state, rows_ws);
}

bool lex_shape_ok(int32_t S, int32_t beam, int32_t n_phr, int32_t V) { return S >= 0 && beam >= 1 && beam <= LX_MAX && V >= 1 && n_phr >= 0 && n_phr <= LEX_MAX_PHR; }

}  // namespace

extern "C" {

int64_t CC_API(cc_beam_lex_ws_bytes)(int32_t S, int32_t beam, int32_t n_phr, int32_t V) {
    if (!lex_shape_ok(S, beam, n_phr, V)) return CC_ERR_ARG;
    if (V > LX_VMAX) return CC_ERR_SHAPE;
    return (int64_t)S * beam * (2 + (int64_t)lx_row_words(beam, n_phr)) * (int64_t)sizeof(float) + 512;
}

int CC_API(cc_beam_lex_step)(int32_t S, int32_t beam, int32_t V, const float* logits, int64_t ldl, float temperature, int32_t first,
                             int32_t stop_token, const int32_t* phrases, int32_t n_phr, int32_t phr_len, float* scores, float* seq_lengths,
                             uint8_t* has_stopped, int32_t* lex_state, int32_t* next_tokens, int32_t* src_rows, void* ws, void* stream) {
    if (!lex_shape_ok(S, beam, n_phr, V) || ldl < V || temperature != temperature || !logits || !scores || !seq_lengths || !has_stopped ||
        !lex_state || !next_tokens || !src_rows || !ws || (n_phr > 0 && (!phrases || phr_len < 1 || phr_len > LEX_MAX_LEN)))
        return CC_ERR_ARG;
    if (V > LX_VMAX) return CC_ERR_SHAPE;
    if (S == 0) return CC_OK;
    hipStream_t st = S_(stream);
    const float inv_temp = 1.0f / (temperature > 0.f ? temperature : 1.0f);   // as cc_beam_step
    if (n_phr == 0) { phrases = nullptr; phr_len = 1; }
    float* rs = static_cast<float*>(ws);
    float* rows_ws = rs + (size_t)S * beam * 2;
    // as cc_beam_step: step 0 reads only row 0 of every sample, but computing all rows' statistics is harmless and uniform
    launch_rowstats(st, logits, ldl, S * beam, V, inv_temp, rs);
    const int blocks = first ? S : S * beam;
#define LEX_ROWS(K) launch_lex_rows<K>(st, blocks, logits, ldl, beam, V, inv_temp, first, stop_token, phrases, n_phr, phr_len, rs, scores, seq_lengths, has_stopped, lex_state, rows_ws)
    switch (beam) {
        case 1: LEX_ROWS(1); break;
        case 2: LEX_ROWS(2); break;
        case 3: LEX_ROWS(3); break;
        case 4: LEX_ROWS(4); break;
        case 5: LEX_ROWS(5); break;
        case 8: LEX_ROWS(8); break;
        default: LEX_ROWS(LX_MAX); break;   // 6, 7, 9 .. 16
    }
#undef LEX_ROWS
    hipLaunchKernelGGL(k_lex_final, dim3(S), dim3(64), 0, st, beam, V, first, stop_token, phrases, n_phr, phr_len, rows_ws, scores, seq_lengths,
                       has_stopped, lex_state, next_tokens, src_rows);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // extern "C"
