// What the caption metrics share (cider.hip: CIDEr-D; metrics.hip: BLEU and ROUGE-L): one workgroup of CD_T threads per candidate, the
// candidate (int64) and its image's references (int32) in LDS, n-grams compared exactly, token by token.  Moved here from cider.hip as it
// stood; device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace cc_caption {

constexpr int CD_T = 256;                    // threads per candidate; >= CD_LMAX: one caption position per thread
constexpr int CD_W = CD_T / 64;
constexpr int CD_LMAX = 256;                 // cand_len and Lr
constexpr int CD_REFMAX = 4096;              // Rmax * Lr: the references of one image in LDS (16 KiB)

template <int N, class A, class B>
__device__ __forceinline__ bool cd_eq(const A* a, const B* b) {
    bool e = true;
#pragma unroll
    for (int k = 0; k < N; k++) e = e && ((long long)a[k] == (long long)b[k]);
    return e;
}

// occurrences of the n-gram g[0..N) in x[0..L); *before = occurrences that start before position `upto`
template <int N, class A, class B>
__device__ __forceinline__ int cd_count(const A* g, const B* x, int L, int upto, int* before) {
    int tf = 0, bf = 0;
    for (int j = 0; j + N <= L; j++) {
        const int m = cd_eq<N>(g, x + j) ? 1 : 0;
        tf += m;
        bf += j < upto ? m : 0;
    }
    *before = bf;
    return tf;
}

// Candidate c into cw[0 .. cand_len) and the R rows in use of image g into rw[0 .. R * Lr), by the whole workgroup; returns the candidate's
// length to every thread.  s_len: one int of LDS.  Ends with a barrier: cw, rw and the length are published.
__device__ __forceinline__ int cd_load_captions(const long long* __restrict__ cand, int c, int cand_len, long long cand_ld, int stop_token,
                                                int count_stop, const int* __restrict__ refs, int g, int Rmax, int Lr, int R, long long* cw,
                                                int* rw, int* s_len) {
    const int tid = threadIdx.x;
    // the candidate: to its first stop token (kept with count_stop), else its first negative id, else cand_len
    if (tid == 0) *s_len = cand_len;
    __syncthreads();
    for (int i = tid; i < cand_len; i += CD_T) {
        const long long t = cand[(size_t)c * cand_ld + i];
        cw[i] = t;
        if (t < 0) atomicMin(s_len, i);
        else if (stop_token >= 0 && t == (long long)stop_token) atomicMin(s_len, count_stop ? i + 1 : i);
    }
    const int* rg = refs + (size_t)g * Rmax * Lr;
    for (int i = tid; i < R * Lr; i += CD_T) rw[i] = rg[i];
    __syncthreads();
    return *s_len;
}

}  // namespace cc_caption
