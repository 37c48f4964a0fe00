// CIDEr-D (Vedantam et al., 2015; the clipped, length-penalised form the reference's eval/pycocoevalcap/cider/cider_scorer.py computes) over
// TOKEN IDS, as the reward of self-critical training (include/clipcap_hip.h cc_cider_score; DESIGN.md states the metric).  Words are token
// ids: no detokenising, no PTB tokenizer.  One launch, one workgroup of CD_T threads per candidate; the candidate and its image's
// references sit in LDS.
//   - tf and first occurrence: the n-gram at position i is compared exactly, token by token, against every position of its own caption;
//     the number of matches is its tf and "no match before i" makes i the position that counts for it.  The same comparison against a
//     reference gives that reference's tf.  No hashing of captions, no sorting: a few thousand compares per n-gram out of LDS.
//   - idf: one probe of the corpus table (cider_table.h) per first-occurrence n-gram; a miss, or an n-gram that cannot be packed (a
//     token id >= 65535), gets log_ndocs.
//   - the references' norms are computed here too, per candidate: they are a few thousand compares each.
//   - every sum is taken in a fixed order: a thread's positions ascending, the wave's butterfly, the waves in index order, the references
//     in index order.  No floating-point atomics: the same input gives the same bits on every run.
//   - the sums over n-grams are fp32 (products of small exact integers and fp32 idf values, none negative); the few scalars per
//     (reference, n) — two square roots, a quotient, the Gaussian penalty — and the sum over references are fp64, rounded once to fp32.
// fp32 / integer work only: built once (Makefile SRCS_ONCE).
#include "layout.h"
#include "cider_table.h"
#include "caption_lds.h"

using namespace CC_NS;
using namespace cc_cider;
using namespace cc_caption;

namespace {

struct CdTable {
    const uint64_t* keys;
    const float* idf;
    int64_t cap;
    float miss;
    template <class T>
    __device__ __forceinline__ float operator()(const T* g, int n) const { return cider_table_find(keys, idf, cap, ct_pack(g, n), miss); }
};

// the candidate's own pass for one n: ctf[i] = tf where position i is the n-gram's first occurrence, else 0; cidf[i] = its idf; returns
// this thread's share of norm_c,n^2
template <int N>
__device__ __forceinline__ float cd_cand_pass(const long long* cw, int Lc, const CdTable& tab, int* ctf, float* cidf) {
    float s = 0.f;
    for (int i = threadIdx.x; i < CD_LMAX; i += CD_T) {
        int tf = 0;
        float idf = 0.f;
        if (i + N <= Lc) {
            int before;
            tf = cd_count<N>(cw + i, cw, Lc, i, &before);
            if (before) tf = 0;
            else { idf = tab(cw + i, N); const float v = (float)tf * idf; s += v * v; }
        }
        ctf[i] = tf;
        cidf[i] = idf;
    }
    return s;
}

// one reference, one n: this thread's shares of sum min(v_c, v_r) v_r (over the candidate's n-grams) and of norm_r,n^2
template <int N>
__device__ __forceinline__ void cd_ref_pass(const long long* cw, int Lc, const int* rw, int Lr, const CdTable& tab, const int* ctf,
                                            const float* cidf, float* val, float* nr2) {
    float v = 0.f, q = 0.f;
    for (int i = threadIdx.x; i + N <= Lc; i += CD_T) {
        const int tfc = ctf[i];
        if (!tfc) continue;
        int before;
        const int tfr = cd_count<N>(cw + i, rw, Lr, 0, &before);
        const float idf = cidf[i], vc = (float)tfc * idf, vr = (float)tfr * idf;
        v += fminf(vc, vr) * vr;
    }
    for (int i = threadIdx.x; i + N <= Lr; i += CD_T) {
        int before;
        const int tfr = cd_count<N>(rw + i, rw, Lr, i, &before);
        if (before) continue;
        const float vr = (float)tfr * tab(rw + i, N);
        q += vr * vr;
    }
    *val = v;
    *nr2 = q;
}

// the block's sums of K values per thread, in a fixed order, to every thread.  red: [K][CD_W]
template <int K>
__device__ __forceinline__ void cd_block_sum(float (&x)[K], float* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; k++)
        for (int o = 32; o > 0; o >>= 1) x[k] += __shfl_xor(x[k], o, 64);
    __syncthreads();                                    // the previous round's readers are done with red
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; k++) red[k * CD_W + wave] = x[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        float s = red[k * CD_W];
        for (int w = 1; w < CD_W; w++) s += red[k * CD_W + w];
        x[k] = s;
    }
}

__global__ __launch_bounds__(CD_T) void k_cider_score(const long long* __restrict__ cand, int cand_len, long long cand_ld, int stop_token,
                                                      int count_stop, const int* __restrict__ cand_group, const int* __restrict__ refs, int G,
                                                      int Rmax, int Lr, const int* __restrict__ ref_count, CdTable tab, double inv_2s2,
                                                      float* __restrict__ out) {
    __shared__ long long cw[CD_LMAX + CT_NMAX];         // (the pad is never read: every n-gram ends inside its caption)
    __shared__ int rw[CD_REFMAX + CT_NMAX];
    __shared__ int ctf[CT_NMAX][CD_LMAX];
    __shared__ float cidf[CT_NMAX][CD_LMAX];
    __shared__ float red[8 * CD_W];
    __shared__ int s_len;
    const int c = blockIdx.x, tid = threadIdx.x;
    const int g = cand_group ? cand_group[c] : c % G;
    if (g < 0 || g >= G) {                              // block-uniform
        if (tid == 0) out[c] = 0.f;
        return;
    }
    int R = ref_count ? ref_count[g] : Rmax;
    R = R < 0 ? 0 : R > Rmax ? Rmax : R;
    const int Lc = cd_load_captions(cand, c, cand_len, cand_ld, stop_token, count_stop, refs, g, Rmax, Lr, R, cw, rw, &s_len);
    float nc[4];
    nc[0] = cd_cand_pass<1>(cw, Lc, tab, ctf[0], cidf[0]);
    nc[1] = cd_cand_pass<2>(cw, Lc, tab, ctf[1], cidf[1]);
    nc[2] = cd_cand_pass<3>(cw, Lc, tab, ctf[2], cidf[2]);
    nc[3] = cd_cand_pass<4>(cw, Lc, tab, ctf[3], cidf[3]);
    cd_block_sum(nc, red);                              // (its barriers also publish ctf / cidf)
    double normc[4];
    for (int n = 0; n < 4; n++) normc[n] = sqrt((double)nc[n]);
    const int lenc = Lc > 0 ? Lc - 1 : 0;               // the reference's length counts bigrams
    double score = 0.0;
    for (int r = 0; r < R; r++) {
        const int* row = rw + r * Lr;
        __syncthreads();                                // the previous reference's s_len has been read by everyone
        if (tid == 0) s_len = Lr;
        __syncthreads();
        if (tid < Lr && row[tid] < 0) atomicMin(&s_len, tid);
        __syncthreads();
        const int Lrr = s_len;
        float x[8];
        cd_ref_pass<1>(cw, Lc, row, Lrr, tab, ctf[0], cidf[0], &x[0], &x[4]);
        cd_ref_pass<2>(cw, Lc, row, Lrr, tab, ctf[1], cidf[1], &x[1], &x[5]);
        cd_ref_pass<3>(cw, Lc, row, Lrr, tab, ctf[2], cidf[2], &x[2], &x[6]);
        cd_ref_pass<4>(cw, Lc, row, Lrr, tab, ctf[3], cidf[3], &x[3], &x[7]);
        cd_block_sum(x, red);
        double sum = 0.0;
        for (int n = 0; n < 4; n++) {
            double v = (double)x[n];
            const double normr = sqrt((double)x[4 + n]);
            if (normc[n] != 0.0 && normr != 0.0) v /= normc[n] * normr;
            sum += v;
        }
        const double d = (double)(lenc - (Lrr > 0 ? Lrr - 1 : 0));
        score += exp(-(d * d) * inv_2s2) * sum;
    }
    if (tid == 0) out[c] = R > 0 ? (float)(score * 10.0 / (4.0 * (double)R)) : 0.f;
}

}  // namespace

extern "C" {

int CC_API(cc_cider_score)(const int64_t* cand, int32_t C, int32_t cand_len, int64_t cand_ld, int32_t stop_token, int32_t count_stop,
                           const int32_t* cand_group, const int32_t* refs, int32_t G, int32_t Rmax, int32_t Lr, const int32_t* ref_count,
                           const uint64_t* tab_keys, const float* tab_idf, int64_t cap, float log_ndocs, float sigma, float* out, void* stream) {
    if (C < 0 || cand_len < 0 || cand_ld < cand_len || G < 1 || Rmax < 1 || Lr < 1 || !ct_pow2(cap)) return CC_ERR_ARG;
    if (!(sigma > 0.f) || !(sigma < INFINITY) || !(log_ndocs > -INFINITY && log_ndocs < INFINITY)) return CC_ERR_ARG;      // NaN fails every comparison
    if (!cand_group && C % G != 0) return CC_ERR_ARG;
    if (C == 0) return CC_OK;                           // nothing to score: nothing is launched
    if (!cand || !refs || !tab_keys || !tab_idf || !out) return CC_ERR_ARG;
    if (cand_len > CD_LMAX || Lr > CD_LMAX || (int64_t)Rmax * Lr > CD_REFMAX || stop_token >= CT_TOKEN_LIMIT) return CC_ERR_SHAPE;
    const CdTable tab{tab_keys, tab_idf, cap, log_ndocs};
    hipLaunchKernelGGL(k_cider_score, dim3(C), dim3(CD_T), 0, S_(stream), reinterpret_cast<const long long*>(cand), cand_len,
                       (long long)cand_ld, stop_token, count_stop != 0 ? 1 : 0, cand_group, refs, G, Rmax, Lr, ref_count, tab,
                       1.0 / (2.0 * (double)sigma * (double)sigma), out);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

// the table of cc_cider_score, built in HOST memory (host-only: no device is touched)
int CC_API(cc_cider_table_build)(const uint64_t* keys, const float* idf, int64_t n, uint64_t* tab_keys, float* tab_idf, int64_t cap) {
    return cider_table_build(keys, idf, n, tab_keys, tab_idf, cap) == 0 ? CC_OK : CC_ERR_ARG;
}

}  // extern "C"
