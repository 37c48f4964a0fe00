// Row state of lexically constrained beam search (include/clipcap_hip.h cc_beam_lex_step): the packing, the transition and tokens_met, one
// definition each.  Plain C++, no HIP include: lexbeam.hip uses it on the device and tests/lex_state_check.cpp on the host.
//   state  : bits 0-7 met (bit c: phrase c has been produced) | bits 8-11 cur + 1 (the phrase in progress, 0 = none) | bits 12-15 pos (the
//            tokens of that phrase matched so far).  0 is the initial state.
//   table  : one sample's phrases, int32 [n_phr][phr_len], -1 after a phrase's last token; phrase c exists iff table[c][0] >= 0.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define LEX_HD __host__ __device__ inline
#else
#define LEX_HD inline
#endif

constexpr int LEX_MAX_PHR = 8;   // phrases per sample
constexpr int LEX_MAX_LEN = 8;   // tokens per phrase

LEX_HD int lex_met(int32_t state) { return state & 0xff; }
LEX_HD int lex_cur(int32_t state) { return ((state >> 8) & 0xf) - 1; }   // -1: no phrase in progress
LEX_HD int lex_pos(int32_t state) { return (state >> 12) & 0xf; }
LEX_HD int32_t lex_pack(int met, int cur, int pos) { return (int32_t)((met & 0xff) | (((cur + 1) & 0xf) << 8) | ((pos & 0xf) << 12)); }

// a phrase's length: the index of its first negative entry, or phr_len
LEX_HD int lex_phrase_len(const int32_t* phrase, int phr_len) {
    int n = 0;
    while (n < phr_len && phrase[n] >= 0) n++;
    return n;
}

// the mask of the sample's existing phrases
LEX_HD int lex_full(const int32_t* table, int n_phr, int phr_len) {
    int full = 0;
    for (int c = 0; c < n_phr; c++) full |= table[c * phr_len] >= 0 ? 1 << c : 0;
    return full;
}

// The state after token v from a parent that has not stopped.  A phrase in progress goes on if v is its next token (and is met when that
// was its last); otherwise the progress is dropped, and the lowest-index unmet phrase that begins with v starts.  No fallback to a shorter
// partial match.
LEX_HD int32_t lex_next(int32_t state, int32_t v, const int32_t* table, int n_phr, int phr_len) {
    const int met = lex_met(state), cur = lex_cur(state), pos = lex_pos(state);
    if (v < 0) return lex_pack(met, -1, 0);
    if (cur >= 0 && cur < n_phr && pos < phr_len && table[cur * phr_len + pos] == v) {
        const int len = lex_phrase_len(table + cur * phr_len, phr_len);
        return pos + 1 >= len ? lex_pack(met | 1 << cur, -1, 0) : lex_pack(met, cur, pos + 1);
    }
    for (int c = 0; c < n_phr; c++) {
        if ((met >> c & 1) || table[c * phr_len] != v) continue;
        return lex_phrase_len(table + c * phr_len, phr_len) == 1 ? lex_pack(met | 1 << c, -1, 0) : lex_pack(met, c, 1);
    }
    return lex_pack(met, -1, 0);
}

// the summed lengths of the met phrases, plus pos when a phrase is in progress
LEX_HD int lex_tokens_met(int32_t state, const int32_t* table, int n_phr, int phr_len) {
    const int met = lex_met(state);
    int n = lex_cur(state) >= 0 ? lex_pos(state) : 0;
    for (int c = 0; c < n_phr; c++)
        if (met >> c & 1) n += lex_phrase_len(table + c * phr_len, phr_len);
    return n;
}
