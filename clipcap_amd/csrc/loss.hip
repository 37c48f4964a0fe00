// The lm_head loss rows for gfx950: cross-entropy and scoring over the lm_head partials, the logits gradient, and the row helpers of
// the exponential-form lm_head.
#include "kernels.h"

namespace CC_NS {

// ------------------------------------------------------------------------------------------------------------
// Cross-entropy over the lm_head partials (clipcap/model/model.py:108-109: ignore_index=0, mean over kept targets).
// k_ce_rows: lse[row] from the per-64-column (max,sumexp) partials; row loss = lse - target_logit for kept rows;
//            stats[0] += sum of kept row losses, stats[1] += number of kept rows.
// k_ce_dlogits: in place over the bf16 logits: dl = (softmax - onehot) * (kept ? 1/denom : 0); padding columns -> 0.
// ------------------------------------------------------------------------------------------------------------
// one wave folds one row's partials: (m, s) with sum over the row's real columns of exp(x) = s exp(m), valid in every lane
// (shared by k_ce_rows and k_score_rows: one order of operations, one lse)
__device__ __forceinline__ void ce_row_fold(const float* __restrict__ pmax, const float* __restrict__ psum, int npart, int row, int lane,
                                            float& m, float& s) {
    m = -INFINITY;
    s = 0.f;
    if (npart <= 64 * 16) {
        // all partials of the row are requested at once (one round trip instead of one per 64 partials, and no second read of the maxima)
        float pm[16], ps[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int p = lane + 64 * i;
            const bool ok = p < npart;
            const size_t at = (size_t)row * npart + min(p, npart - 1);      // clamped address + select: the loads stay one batch
            const float a = pmax[at], b = psum[at];
            pm[i] = ok ? a : -INFINITY;
            ps[i] = ok ? b : 0.f;
            m = fmaxf(m, pm[i]);
        }
        m = wave_max(m);
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (pm[i] != -INFINITY) s += ps[i] * __expf(pm[i] - m);
    } else {
        for (int p = lane; p < npart; p += 64) m = fmaxf(m, pmax[(size_t)row * npart + p]);
        m = wave_max(m);
        for (int p = lane; p < npart; p += 64) {
            const float pm = pmax[(size_t)row * npart + p];
            if (pm != -INFINITY) s += psum[(size_t)row * npart + p] * __expf(pm - m);
        }
    }
    s = wave_sum(s);
}
// lse of one row from its partials, valid in every lane
__device__ __forceinline__ float ce_row_lse(const float* __restrict__ pmax, const float* __restrict__ psum, int npart, int row, int lane) {
    float m, s;
    ce_row_fold(pmax, psum, npart, row, lane, m, s);
    return m + logf(s);
}
__global__ __launch_bounds__(256) void k_ce_rows(const float* __restrict__ pmax, const float* __restrict__ psum, int npart,
                                                 const int* __restrict__ target, const float* __restrict__ tgt_logit,
                                                 float* __restrict__ lse, float* __restrict__ row_loss, int M) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float l = ce_row_lse(pmax, psum, npart, row, lane);
    if (lane == 0) {
        lse[row] = l;
        row_loss[row] = (target[row] != 0) ? l - tgt_logit[row] : 0.f;
    }
}
// stats[0] = sum of kept-row losses, stats[1] = kept rows — one block, fixed summation order (deterministic, no atomics).
// WT (per-row loss weights, row_factor): stats[0] = the sum of rw[i] * row_loss[i] over the kept rows, stats[2] = the plain sum in the
// order stats[0] has without weights; a kept row of weight 0 still counts in stats[1].  row_loss itself stays the plain row loss.
template <bool WT>
__global__ __launch_bounds__(1024) void k_ce_stats(const float* __restrict__ row_loss, const int* __restrict__ target,
                                                   const float* __restrict__ rw, float* __restrict__ stats, int M) {
    __shared__ float sl[16], sc[16], sp[WT ? 16 : 1];
    float a = 0.f, c = 0.f, p = 0.f;
    for (int i = threadIdx.x; i < M; i += 1024) {
        const int t = target[i];
        const float l = row_loss[i];
        a += WT ? row_factor<true>(t, l, rw, i) : l;
        c += (t != 0) ? 1.f : 0.f;
        if (WT) p += l;
    }
    a = wave_sum(a);
    c = wave_sum(c);
    if (WT) p = wave_sum(p);
    if ((threadIdx.x & 63) == 0) {
        sl[threadIdx.x >> 6] = a;
        sc[threadIdx.x >> 6] = c;
        if (WT) sp[threadIdx.x >> 6] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float ta = 0.f, tc = 0.f, tp = 0.f;
        for (int w = 0; w < 16; w++) {
            ta += sl[w];
            tc += sc[w];
            if (WT) tp += sp[w];
        }
        stats[0] = ta;
        stats[1] = tc;
        if (WT) stats[2] = tp;
    }
}
int ce_rows(const float* pmax, const float* psum, int npart, const int* target, const float* tgt_logit, float* lse, float* row_loss,
            float* stats, int M, hipStream_t st, const float* row_weight) {
    if (M <= 0) return CC_OK;
    hipLaunchKernelGGL(k_ce_rows, dim3((M + 3) / 4), dim3(256), 0, st, pmax, psum, npart, target, tgt_logit, lse, row_loss, M);
    if (row_weight) hipLaunchKernelGGL(k_ce_stats<true>, dim3(1), dim3(1024), 0, st, row_loss, target, row_weight, stats, M);
    else hipLaunchKernelGGL(k_ce_stats<false>, dim3(1), dim3(1024), 0, st, row_loss, target, nullptr, stats, M);
    return CC_OK;
}

// Scoring (cc_lmhead_score): token_logprob[row] = tgt_logit - lse for kept rows, 0 for the others; lse from the same fold as k_ce_rows.
__global__ __launch_bounds__(256) void k_score_rows(const float* __restrict__ pmax, const float* __restrict__ psum, int npart,
                                                    const int* __restrict__ keep, const float* __restrict__ tgt_logit,
                                                    float* __restrict__ lse, float* __restrict__ token_logprob, int M) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float l = ce_row_lse(pmax, psum, npart, row, lane);
    if (lane == 0) {
        lse[row] = l;
        token_logprob[row] = keep[row] ? tgt_logit[row] - l : 0.f;
    }
}
// sample_stats[b] = {sum of the sample's kept log-probs, kept count}: one wave per sample, lane j adds rows j, j + 64, ... in that order,
// then the fixed wave tree (deterministic, no atomics)
__global__ __launch_bounds__(256) void k_score_samples(const float* __restrict__ token_logprob, const int* __restrict__ keep,
                                                       float* __restrict__ sample_stats, int B, int cap) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float a = 0.f, c = 0.f;
    for (int i = lane; i < cap; i += 64) {
        a += token_logprob[(size_t)b * cap + i];
        c += keep[(size_t)b * cap + i] ? 1.f : 0.f;
    }
    a = wave_sum(a);
    c = wave_sum(c);
    if (lane == 0) {
        sample_stats[2 * b] = a;
        sample_stats[2 * b + 1] = c;
    }
}
int score_rows(const float* pmax, const float* psum, int npart, const int* keep, const float* tgt_logit, float* lse, float* token_logprob,
               float* sample_stats, int B, int cap, hipStream_t st) {
    const int M = B * cap;
    if (M <= 0) return CC_OK;
    hipLaunchKernelGGL(k_score_rows, dim3((M + 3) / 4), dim3(256), 0, st, pmax, psum, npart, keep, tgt_logit, lse, token_logprob, M);
    hipLaunchKernelGGL(k_score_samples, dim3((B + 3) / 4), dim3(256), 0, st, token_logprob, keep, sample_stats, B, cap);
    return CC_OK;
}

// img (bf16x3 build): the gradient is written as the [hi | hi | lo] operand image of the lm_head's input-gradient GEMM (rows of 3 ld
// 16-bit elements) into img instead of in place over the fp32 logits
template <bool WT>
__global__ __launch_bounds__(256) void k_ce_dlogits(act_t* __restrict__ logits, int ld, int V, const int* __restrict__ target,
                                                    const float* __restrict__ lse, const float* __restrict__ denom,
                                                    const float* __restrict__ loss_scale, const float* __restrict__ rw, int M,
                                                    op16_t* __restrict__ img) {
    const int col = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (col >= ld) return;
    const float inv = (loss_scale ? loss_scale[0] : 1.0f) / fmaxf(denom[0], 1.0f);
    for (int row = blockIdx.y; row < M; row += gridDim.y) {
        const int t = target[row];
        const float l = lse[row];
        // WT: the factor's magnitude; its sign goes onto the GEMMs' other side (k_lm_rowsign), so that the matrix cores, whose
        // accumulation is not symmetric under negation of an operand, see the operand of the row with the weight's sign dropped
        const float w = WT ? fabsf(row_factor<WT>(t, inv, rw, row)) : row_factor<WT>(t, inv, rw, row);
        act_t* p = logits + (size_t)row * ld + col;
        float f[8];
        act_ld8(p, f);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int c = col + e;
            f[e] = (c < V) ? (__expf(f[e] - l) - (c == t ? 1.f : 0.f)) * w : 0.f;
        }
#if CC_OP == 2
        if (img) {
            uint4 hi, lo;
            x3_pair8(f, hi, lo);
            x3_store(img + (size_t)row * 3 * ld + col, ld, 0, 0, hi, lo);
            continue;
        }
#endif
        act_st8(p, f);
    }
}
int ce_dlogits(act_t* logits, int ld, int V, const int* target, const float* lse, const float* denom, const float* loss_scale, int M,
               hipStream_t st, op16_t* img, const float* row_weight) {
    if (ld & 7) return CC_ERR_SHAPE;
    if (M <= 0) return CC_OK;
    const dim3 grid((ld / 8 + 255) / 256, std::min(M, 32768));
    if (row_weight) hipLaunchKernelGGL(k_ce_dlogits<true>, grid, dim3(256), 0, st, logits, ld, V, target, lse, denom, loss_scale, row_weight, M, img);
    else hipLaunchKernelGGL(k_ce_dlogits<false>, grid, dim3(256), 0, st, logits, ld, V, target, lse, denom, loss_scale, nullptr, M, img);
    return CC_OK;
}

// ---- exponential form of the lm_head outputs (gemm.hip.h EpiLMHead): row helpers, one wave per row ----
// eight elements of the wte operand arena at element offset `at`, as floats; bf16x3: of the fp32 master row (what hi + lo stand for)
__device__ __forceinline__ void ld_wte8(const op16_t* __restrict__ wte, size_t at, float (&b)[8]) {
#if CC_OP == 2
    act_ld8(reinterpret_cast<const float*>(wte) + at, b);
#else
    unpack8(*reinterpret_cast<const uint4*>(wte + at), b);
#endif
}
__global__ __launch_bounds__(256) void k_lm_tgt_ref(const act_t* __restrict__ hf, const op16_t* __restrict__ wte, int D, const int* __restrict__ target,
                                                    float* __restrict__ cref, int M) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const act_t* h = hf + (size_t)row * D;
    const size_t w = (size_t)target[row] * D;
    float acc = 0.f;
    for (int d = lane * 8; d < D; d += 512) {
        float a[8], b[8];
        act_ld8(h + d, a);
        ld_wte8(wte, w + d, b);
#pragma unroll
        for (int e = 0; e < 8; e++) acc += a[e] * b[e];
    }
    acc = wave_sum(acc);
    if (lane == 0) cref[row] = acc;
}
int lm_tgt_ref(const act_t* hf, const op16_t* wte, int D, const int* target, float* cref, int M, hipStream_t st) {
    if (D & 7) return CC_ERR_SHAPE;
    if (M <= 0) return CC_OK;
    hipLaunchKernelGGL(k_lm_tgt_ref, dim3((M + 3) / 4), dim3(256), 0, st, hf, wte, D, target, cref, M);
    return CC_OK;
}
// w: row_factor, of either sign with weights; a kept row of weight 0 has w == 0 and so r == 0, as an ignored row has — its gradient IS zero
template <bool WT>
__global__ void k_lm_rowfac(const float* __restrict__ cref, const float* __restrict__ lse, const int* __restrict__ target,
                            const float* __restrict__ denom, const float* __restrict__ loss_scale, const float* __restrict__ rw,
                            float* __restrict__ fac, int M) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float inv = (loss_scale ? loss_scale[0] : 1.0f) / fmaxf(denom[0], 1.0f);
    const float w = row_factor<WT>(target[i], inv, rw, i);
    fac[2 * i] = w != 0.f ? __expf(cref[i] - lse[i]) * w : 0.f;
    fac[2 * i + 1] = w;
}
int lm_rowfac(const float* cref, const float* lse, const int* target, const float* denom, const float* loss_scale, float* fac, int M, hipStream_t st,
              const float* row_weight) {
    if (M <= 0) return CC_OK;
    if (row_weight) hipLaunchKernelGGL(k_lm_rowfac<true>, dim3((M + 255) / 256), dim3(256), 0, st, cref, lse, target, denom, loss_scale, row_weight, fac, M);
    else hipLaunchKernelGGL(k_lm_rowfac<false>, dim3((M + 255) / 256), dim3(256), 0, st, cref, lse, target, denom, loss_scale, nullptr, fac, M);
    return CC_OK;
}
// logit form with weights: fac[m] = {s, 0}, s = -1 where the row factor (row_factor: loss_scale / max(denom, 1) * rw[m]) is negative, else 1.
// k_ce_dlogits<true> puts the factor's magnitude into d logits; lm_scale_rows puts s onto the rows of d hf after the input-gradient GEMM and
// onto the hf rows the tied weight-gradient GEMM reads.  Negating a weight then negates its row's gradient bit for bit.
__global__ void k_lm_rowsign(const int* __restrict__ target, const float* __restrict__ denom, const float* __restrict__ loss_scale,
                             const float* __restrict__ rw, float* __restrict__ fac, int M) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float inv = (loss_scale ? loss_scale[0] : 1.0f) / fmaxf(denom[0], 1.0f);
    fac[2 * i] = row_factor<true>(target[i], inv, rw, i) < 0.f ? -1.f : 1.f;
    fac[2 * i + 1] = 0.f;
}
int lm_rowsign(const int* target, const float* denom, const float* loss_scale, const float* row_weight, float* fac, int M, hipStream_t st) {
    if (M <= 0) return CC_OK;
    hipLaunchKernelGGL(k_lm_rowsign, dim3((M + 255) / 256), dim3(256), 0, st, target, denom, loss_scale, row_weight, fac, M);
    return CC_OK;
}
// MODE 0: dhf = r dhf - w wte[t];  1: out = r hf;  2: io = r io (in place)
template <int MODE>
__global__ __launch_bounds__(256) void k_lm_rows(act_t* __restrict__ io, const act_t* __restrict__ hf, const float* __restrict__ fac,
                                                 const int* __restrict__ target, const op16_t* __restrict__ wte, int D, int M) {
    const int d8n = D >> 3;
    const size_t total = (size_t)M * d8n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / d8n), c = (int)(i % d8n) * 8;
        const float r = fac[2 * row], w = fac[2 * row + 1];
        float v[8];
        if (MODE == 0) {
            float b[8];
            act_ld8(io + (size_t)row * D + c, v);
            ld_wte8(wte, (size_t)target[row] * D + c, b);
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = r * v[e] - w * b[e];
            act_st8(io + (size_t)row * D + c, v);
        } else {
            act_ld8((MODE == 2 ? io : hf) + (size_t)row * D + c, v);
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] *= r;
            act_st8(io + (size_t)row * D + c, v);
        }
    }
}
template <int MODE>
static int lm_rows_launch(act_t* io, const act_t* hf, const float* fac, const int* target, const op16_t* wte, int D, int M, hipStream_t st) {
    if (D & 7) return CC_ERR_SHAPE;
    const size_t total = (size_t)M * (D >> 3);
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_lm_rows<MODE>, flat_grid(total, 256, 4096), dim3(256), 0, st, io, hf, fac, target, wte, D, M);
    return CC_OK;
}
int lm_dgrad_fix(act_t* dhf, const float* fac, const int* target, const op16_t* wte, int D, int M, hipStream_t st) {
    return lm_rows_launch<0>(dhf, nullptr, fac, target, wte, D, M, st);
}
int lm_scale_rows(const act_t* hf, const float* fac, act_t* out, int D, int M, hipStream_t st) {
    return lm_rows_launch<1>(out, hf, fac, nullptr, nullptr, D, M, st);
}
int lm_scale_rows_inplace(act_t* x, const float* fac, int D, int M, hipStream_t st) {
    return lm_rows_launch<2>(x, nullptr, fac, nullptr, nullptr, D, M, st);
}

// Targets of the caption rows: target[b*cap + c] = max(tokens[b,c], 0) (model.py:103-104); row_map[b*cap+c] = b*T + L-1+c.
__global__ void k_ce_targets(const long long* __restrict__ tokens, int* __restrict__ target, int* __restrict__ row_map, int B, int cap,
                             int L, int T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * cap) return;
    const int b = i / cap, c = i % cap;
    long long id = tokens[i];
    target[i] = id < 0 ? 0 : (int)id;
    row_map[i] = b * T + L - 1 + c;
}
int ce_targets(const long long* tokens, int* target, int* row_map, int B, int cap, int L, int T, hipStream_t st) {
    if (B * cap <= 0) return CC_OK;
    hipLaunchKernelGGL(k_ce_targets, dim3((B * cap + 255) / 256), dim3(256), 0, st, tokens, target, row_map, B, cap, L, T);
    return CC_OK;
}
// Kept rows of a scoring call, from the ORIGINAL tokens (ce_targets has already mapped the -1 pads to target 0): keep[i] = tokens[i] >= 0,
// and with ignore_zero also tokens[i] != 0 (the training loss's ignore_index = 0, model.py:108-109)
__global__ void k_score_keep(const long long* __restrict__ tokens, int* __restrict__ keep, int n, int ignore_zero) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long id = tokens[i];
    keep[i] = (id >= 0 && !(ignore_zero && id == 0)) ? 1 : 0;
}
int score_keep(const long long* tokens, int* keep, int n, int ignore_zero, hipStream_t st) {
    if (n <= 0) return CC_OK;
    hipLaunchKernelGGL(k_score_keep, dim3((n + 255) / 256), dim3(256), 0, st, tokens, keep, n, ignore_zero);
    return CC_OK;
}

}  // namespace CC_NS
