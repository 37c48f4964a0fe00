// BLEU-1..4 and ROUGE-L over word ids (include/clipcap_hip.h cc_bleu_stats, cc_rouge_l; DESIGN.md states the metrics: the reference's
// eval/pycocoevalcap/bleu/bleu_scorer.py with option "closest" and eval/pycocoevalcap/rouge/rouge.py).  Words are non-negative integers:
// token ids, or the word ids of clipcap_amd.eval.  One launch each, one workgroup of CD_T threads per candidate; the candidate and its
// image's references sit in LDS, loaded and cut by the code cider.hip uses (caption_lds.h).
//   - BLEU: wave w counts the n-grams of n = w + 1.  The n-gram at position i is compared exactly, token by token, against every position
//     of its own caption (its tf; "no match before i" makes i the position that counts for it) and of every reference in use (the largest
//     tf); min of the two is what it adds to correct[n].  No hashing, no table: any id >= 0 is a word.  Integer sums: a lane's positions
//     ascending, the wave's butterfly.  The ten integers are exact; the four sentence scores are fp64 from them, rounded once to fp32.
//   - ROUGE-L: the bit-parallel LCS (Allison & Dix 1986; Hyyro 2004).  One wave takes one reference at a time; lane l holds the
//     candidate's words 64 w + l, w = 0..3.  For each reference word t the four ballots of cand[64 w + lane] == t are the 256-bit match
//     mask M, and  U = V & M;  V = (V + U) | (V & ~U)  with the carry taken across the words.  V starts as all ones; the LCS is the number
//     of zero bits (bits at and above the candidate's length never match, so they stay one).  The masks are wave-uniform: every lane
//     carries the same V.  A wave's references ascending, the waves in index order; P, R and the score are fp64, rounded once.
//   - nothing is added in floating point and the only atomic is the integer LDS minimum of the shared caption load: the same input gives
//     the same bits on every run, and a row does not depend on the other candidates.
// fp64 / integer work only: built once (Makefile SRCS_ONCE).
#include "layout.h"
#include "caption_lds.h"

using namespace CC_NS;
using namespace cc_caption;

namespace {

// the length of one reference row (it ends at its first negative id, else at Lr), to every lane of the calling wave
__device__ __forceinline__ int mt_row_len(const int* row, int Lr) {
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < Lr; base += 64) {
        const int i = base + lane;
        const unsigned long long neg = __ballot(i < Lr && row[i] < 0);
        if (neg) return base + __ffsll((long long)neg) - 1;
    }
    return Lr;
}

__device__ __forceinline__ int mt_wave_sum(int x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ int mt_wave_min(int x) {
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
    return x;
}

// this lane's share of correct[N]: over the positions where an n-gram of the candidate first occurs, min(its tf, its largest tf in a reference)
template <int N>
__device__ __forceinline__ int bl_correct(const long long* cw, int Lc, const int* rw, int Lr, int R, const int* rlen) {
    int sum = 0;
    for (int i = threadIdx.x & 63; i + N <= Lc; i += 64) {
        int before;
        const int tf = cd_count<N>(cw + i, cw, Lc, i, &before);
        if (before) continue;
        int most = 0;
        for (int r = 0; r < R && most < tf; r++) {      // (a reference that reaches tf settles the min)
            int unused;
            most = max(most, cd_count<N>(cw + i, rw + r * Lr, rlen[r], 0, &unused));
        }
        sum += min(tf, most);
    }
    return sum;
}

__global__ __launch_bounds__(CD_T) void k_bleu_stats(const long long* __restrict__ cand, int cand_len, long long cand_ld, int stop_token,
                                                     int count_stop, const int* __restrict__ cand_group, const int* __restrict__ refs, int G,
                                                     int Rmax, int Lr, const int* __restrict__ ref_count, int* __restrict__ stats,
                                                     float* __restrict__ bleu) {
    __shared__ long long cw[CD_LMAX];
    __shared__ int rw[CD_REFMAX];
    __shared__ int rlen[CD_REFMAX];                     // (Rmax reaches CD_REFMAX at Lr = 1)
    __shared__ int s_correct[CD_W];
    __shared__ int s_key[CD_W];
    __shared__ int s_len;
    const int c = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = cand_group ? cand_group[c] : c % G;
    if (g < 0 || g >= G) {                              // block-uniform
        if (tid < 10) stats[(size_t)c * 10 + tid] = 0;
        if (bleu && tid < 4) bleu[(size_t)c * 4 + tid] = 0.f;
        return;
    }
    int R = ref_count ? ref_count[g] : Rmax;
    R = R < 1 ? 1 : R > Rmax ? Rmax : R;
    const int Lc = cd_load_captions(cand, c, cand_len, cand_ld, stop_token, count_stop, refs, g, Rmax, Lr, R, cw, rw, &s_len);
    for (int r = wave; r < R; r += CD_W) {
        const int len = mt_row_len(rw + r * Lr, Lr);
        if (lane == 0) rlen[r] = len;
    }
    __syncthreads();
    // the closest reference length, the shorter on a tie: the smallest (|l - Lc|, l), as one integer (l <= 256 < 512)
    int key = 0x7fffffff;
    for (int r = tid; r < R; r += CD_T) {
        const int l = rlen[r];
        key = min(key, (l > Lc ? l - Lc : Lc - l) * 512 + l);
    }
    key = mt_wave_min(key);
    int corr = wave == 0   ? bl_correct<1>(cw, Lc, rw, Lr, R, rlen)
               : wave == 1 ? bl_correct<2>(cw, Lc, rw, Lr, R, rlen)
               : wave == 2 ? bl_correct<3>(cw, Lc, rw, Lr, R, rlen)
                           : bl_correct<4>(cw, Lc, rw, Lr, R, rlen);
    corr = mt_wave_sum(corr);
    if (lane == 0) {
        s_key[wave] = key;
        s_correct[wave] = corr;
    }
    __syncthreads();
    int k = s_key[0];
    for (int w = 1; w < CD_W; w++) k = min(k, s_key[w]);
    const int reflen = k & 511;
    if (tid < 10) stats[(size_t)c * 10 + tid] = tid == 0 ? Lc : tid == 1 ? reflen : tid < 6 ? max(0, Lc - (tid - 2)) : s_correct[tid - 6];
    if (bleu && tid < 4) {
#pragma clang fp contract(off)
        const double tiny = 1e-15, small = 1e-9;        // the reference scorer's constants
        double p = 1.0;
        for (int n = 0; n <= tid; n++) p *= ((double)s_correct[n] + tiny) / ((double)max(0, Lc - n) + small);
        double b = pow(p, 1.0 / (double)(tid + 1));
        const double ratio = ((double)Lc + tiny) / ((double)reflen + small);
        if (ratio < 1.0) b *= exp(1.0 - 1.0 / ratio);
        bleu[(size_t)c * 4 + tid] = (float)b;
    }
}

// LCS of the candidate (cv[w] = its word 64 w + lane, -1 at and beyond its length; W = the 64-bit words that hold it) and row[0 .. len),
// by one wave, to every lane
template <int W>
__device__ __forceinline__ int rl_lcs(const long long (&cv)[4], const int* row, int len) {
    const int lane = threadIdx.x & 63;
    unsigned long long V[W];
#pragma unroll
    for (int w = 0; w < W; w++) V[w] = ~0ull;
    for (int base = 0; base < len; base += 64) {
        const int mine = base + lane < len ? row[base + lane] : -1;      // 64 reference words in one LDS read; handed round by readlane
        const int nj = min(64, len - base);
        for (int j = 0; j < nj; j++) {
            const long long t = (long long)__builtin_amdgcn_readlane(mine, j);
            unsigned long long carry = 0;
#pragma unroll
            for (int w = 0; w < W; w++) {
                const unsigned long long M = __ballot(cv[w] == t);
                const unsigned long long U = V[w] & M;
                const unsigned long long s = V[w] + U;
                const unsigned long long s2 = s + carry;
                carry = (unsigned long long)(s < U) | (unsigned long long)(s2 < s);
                V[w] = s2 | (V[w] & ~U);
            }
        }
    }
    int zeros = 0;
#pragma unroll
    for (int w = 0; w < W; w++) zeros += __popcll(~V[w]);
    return zeros;
}

__global__ __launch_bounds__(CD_T) void k_rouge_l(const long long* __restrict__ cand, int cand_len, long long cand_ld, int stop_token,
                                                  int count_stop, const int* __restrict__ cand_group, const int* __restrict__ refs, int G,
                                                  int Rmax, int Lr, const int* __restrict__ ref_count, float beta, int* __restrict__ lcs,
                                                  float* __restrict__ out) {
    __shared__ long long cw[CD_LMAX];
    __shared__ int rw[CD_REFMAX];
    __shared__ int s_best[CD_W];
    __shared__ double s_rec[CD_W];
    __shared__ int s_len;
    const int c = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = cand_group ? cand_group[c] : c % G;
    if (g < 0 || g >= G) {                              // block-uniform: no image, so no row is in use
        if (tid == 0) out[c] = 0.f;
        if (lcs)
            for (int r = tid; r < Rmax; r += CD_T) lcs[(size_t)c * Rmax + r] = -1;
        return;
    }
    int R = ref_count ? ref_count[g] : Rmax;
    R = R < 1 ? 1 : R > Rmax ? Rmax : R;
    const int Lc = cd_load_captions(cand, c, cand_len, cand_ld, stop_token, count_stop, refs, g, Rmax, Lr, R, cw, rw, &s_len);
    long long cv[4];
#pragma unroll
    for (int w = 0; w < 4; w++) cv[w] = 64 * w + lane < Lc ? cw[64 * w + lane] : -1ll;
    const int W = (Lc + 63) >> 6;
    int best = 0;                                       // max lcs: P = best / Lc
    double rec = 0.0;                                   // max lcs / L_r (a maximum of correctly rounded quotients: any order gives the same bits)
    for (int r = wave; r < R; r += CD_W) {              // wave-uniform: every lane is active at every ballot
        const int* row = rw + r * Lr;
        const int len = mt_row_len(row, Lr);
        int l = 0;
        if (len > 0) l = W == 1 ? rl_lcs<1>(cv, row, len) : W == 2 ? rl_lcs<2>(cv, row, len) : W == 3 ? rl_lcs<3>(cv, row, len) : W == 4 ? rl_lcs<4>(cv, row, len) : 0;
        if (lcs && lane == 0) lcs[(size_t)c * Rmax + r] = l;
        best = max(best, l);
        if (len > 0) rec = fmax(rec, (double)l / (double)len);
    }
    if (lcs)
        for (int r = R + tid; r < Rmax; r += CD_T) lcs[(size_t)c * Rmax + r] = -1;
    if (lane == 0) {
        s_best[wave] = best;
        s_rec[wave] = rec;
    }
    __syncthreads();
    if (tid == 0) {
#pragma clang fp contract(off)
        for (int w = 1; w < CD_W; w++) {
            best = max(best, s_best[w]);
            rec = fmax(rec, s_rec[w]);
        }
        const double prec = Lc > 0 ? (double)best / (double)Lc : 0.0, b2 = (double)beta * (double)beta;
        out[c] = prec != 0.0 && rec != 0.0 ? (float)(((1.0 + b2) * prec * rec) / (rec + b2 * prec)) : 0.f;
    }
}

// what both entry points decide before anything touches the device; CC_OK with *launch = false: nothing to do
int mt_check(const int64_t* cand, int32_t C, int32_t cand_len, int64_t cand_ld, const int32_t* cand_group, const int32_t* refs, int32_t G,
             int32_t Rmax, int32_t Lr, const void* out, bool* launch) {
    *launch = false;
    if (C < 0 || cand_len < 0 || cand_ld < cand_len || G < 1 || Rmax < 1 || Lr < 1) return CC_ERR_ARG;
    if (!cand_group && C % G != 0) return CC_ERR_ARG;
    if (C == 0) return CC_OK;                           // nothing to score: nothing is launched
    if (!cand || !refs || !out) return CC_ERR_ARG;
    if (cand_len > CD_LMAX || Lr > CD_LMAX || (int64_t)Rmax * Lr > CD_REFMAX) return CC_ERR_SHAPE;
    *launch = true;
    return CC_OK;
}

}  // namespace

extern "C" {

int CC_API(cc_bleu_stats)(const int64_t* cand, int32_t C, int32_t cand_len, int64_t cand_ld, int32_t stop_token, int32_t count_stop,
                          const int32_t* cand_group, const int32_t* refs, int32_t G, int32_t Rmax, int32_t Lr, const int32_t* ref_count,
                          int32_t* stats, float* bleu, void* stream) {
    bool launch;
    CC_TRY(mt_check(cand, C, cand_len, cand_ld, cand_group, refs, G, Rmax, Lr, stats, &launch));
    if (!launch) return CC_OK;
    hipLaunchKernelGGL(k_bleu_stats, dim3(C), dim3(CD_T), 0, S_(stream), reinterpret_cast<const long long*>(cand), cand_len,
                       (long long)cand_ld, stop_token, count_stop != 0 ? 1 : 0, cand_group, refs, G, Rmax, Lr, ref_count, stats, bleu);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int CC_API(cc_rouge_l)(const int64_t* cand, int32_t C, int32_t cand_len, int64_t cand_ld, int32_t stop_token, int32_t count_stop,
                       const int32_t* cand_group, const int32_t* refs, int32_t G, int32_t Rmax, int32_t Lr, const int32_t* ref_count,
                       float beta, int32_t* lcs, float* out, void* stream) {
    if (!(beta > 0.f) || !(beta < INFINITY)) return CC_ERR_ARG;            // NaN fails every comparison
    bool launch;
    CC_TRY(mt_check(cand, C, cand_len, cand_ld, cand_group, refs, G, Rmax, Lr, out, &launch));
    if (!launch) return CC_OK;
    hipLaunchKernelGGL(k_rouge_l, dim3(C), dim3(CD_T), 0, S_(stream), reinterpret_cast<const long long*>(cand), cand_len, (long long)cand_ld,
                       stop_token, count_stop != 0 ? 1 : 0, cand_group, refs, G, Rmax, Lr, ref_count, beta, lcs, out);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // extern "C"
