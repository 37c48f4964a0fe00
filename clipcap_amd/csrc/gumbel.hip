// Stochastic beam search (Kool, van Hoof, Welling, ICML 2019: "Stochastic Beams and Where to Find Them"; not in the reference): the device
// update that turns one step's logits into `beam` continuations sampled WITHOUT replacement (include/clipcap_hip.h cc_beam_gumbel_step).
// Every candidate's log-probability is perturbed with Gumbel noise from a counter-based generator (philox.h: no noise tensor; 16 M draws
// per step at S = 64, beam 5, V = 50257), a child's perturbed value is conditioned on its parent's, and a top-`beam` over the children
// gives the sample.  Two launches, one read of the logits, no atomics:
//   k_gumbel_rows  : one block per live parent row: running softmax pair over x = logit / T, and the row's `beam` best tokens by
//                    y = x + noise.  The conditioned value is non-decreasing in y within a row, so this pruning is exact and the
//                    transform is evaluated for `beam` tokens per row instead of V.
//   k_gumbel_final : one 64-thread block per sample: the transform for at most beam^2 kept candidates, the pick and the commit.
// Built on select.hip.h (cand_better, SoftmaxPair, SortedList, block_argmax, pick_from_list).  No 16-bit operands (fp32 and integer work,
// fp64 for the few kept candidates), so this unit is built once (Makefile).  Plain C++: no inline assembly.
#include "layout.h"
#include "philox.h"
#include "select.hip.h"

using namespace CC_NS;

namespace {

constexpr int GB_MAX = 16;                // widest beam
constexpr int GB_VMAX = 2097152;          // 16 * 2^21 flat indices stay far inside int
constexpr int GR_T = 512;                 // threads per parent row (8 waves), as k_beam_rowstats and k_contrastive_topk
constexpr int GB_HDR = 4;                 // workspace per row: m, sum, kept count, pad | v[beam]

// Standard Gumbel noise from 32 random bits: u = (h + 0.5) / 2^32 in (0, 1), n = -ln(-ln u), a real in (-3.14, 22.9).  u is never formed
// near 1: the upper half of the words goes through log1p of the distance to 1.
__device__ __forceinline__ float gumbel_of_bits(uint32_t h) {
    float e;
    if (h < 0x80000000u) e = -logf(((float)h + 0.5f) * 0x1p-32f);
    else e = -log1pf(-(((float)(0xffffffffu - h) + 0.5f) * 0x1p-32f));
    return -logf(e);
}

__host__ __device__ __forceinline__ size_t gb_row_floats(int beam) { return (size_t)GB_HDR + (size_t)beam; }

// K: length of the register lists (>= the beam width `beam`; 16 serves every width without a compile-time list of its own: the K best
// contain the `beam` best, so the run-time widths need no dynamically indexed list).  VEC: rows are 16-B aligned -> float4 loads.
// A thread covers whole groups of four tokens, so one Philox call feeds four.
template <int K, bool VEC>
__global__ __launch_bounds__(GR_T) void k_gumbel_rows(const float* __restrict__ logits, size_t ldl, int beam, int V, float inv_temp, int first,
                                                      uint64_t seed, int step, const unsigned char* __restrict__ stopped, float* __restrict__ ws) {
    constexpr int NW = GR_T / 64;
    __shared__ float redm[NW], reds[NW], redv[2 * NW];
    __shared__ int redi[2 * NW];
    __shared__ int sel_t[GB_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row = first ? blockIdx.x * beam : blockIdx.x;             // the first step reads row 0 of every sample, under its own index
    if (!first && stopped[row]) return;                                 // block-uniform, before any barrier; the row is not read
    const float* lg = logits + (size_t)row * ldl;
    SortedList<K> top;
    top.clear();
    SoftmaxPair p;
    auto take = [&](float x, float n, int v) {
        if (x > -INFINITY) top.enter(__fadd_rn(x, n), v);               // a banned token is no candidate
    };
    const int NG = (V + 3) >> 2;
    for (int q = tid; q < NG; q += GR_T) {
        float x0, x1, x2, x3;
        if (VEC && 4 * q + 3 < V) {
            const float4 x = reinterpret_cast<const float4*>(lg)[q];
            x0 = x.x * inv_temp; x1 = x.y * inv_temp; x2 = x.z * inv_temp; x3 = x.w * inv_temp;
        } else {                                                        // unaligned rows, and the last group of a row whose V is no multiple of 4
            x0 = lg[4 * q] * inv_temp;
            x1 = 4 * q + 1 < V ? lg[4 * q + 1] * inv_temp : -INFINITY;
            x2 = 4 * q + 2 < V ? lg[4 * q + 2] * inv_temp : -INFINITY;
            x3 = 4 * q + 3 < V ? lg[4 * q + 3] * inv_temp : -INFINITY;
        }
        p.add4(x0, x1, x2, x3);
        const philox4 h = gumbel_bits4(seed, (uint32_t)step, (uint32_t)row, (uint32_t)q);
        take(x0, gumbel_of_bits(h.w[0]), 4 * q);
        take(x1, gumbel_of_bits(h.w[1]), 4 * q + 1);
        take(x2, gumbel_of_bits(h.w[2]), 4 * q + 2);
        take(x3, gumbel_of_bits(h.w[3]), 4 * q + 3);
    }
    // the row's (max, sum): pairs merged across lanes and waves in a fixed order
    p.wave_merge();
    if (lane == 0) { redm[wv] = p.m; reds[wv] = p.sum; }
    __syncthreads();
    p.m = redm[0]; p.sum = reds[0];
    for (int i = 1; i < NW; i++) p.merge(redm[i], reds[i]);
    // `beam` rounds of block arg-max over the list heads (y descending, token ascending); the winner's owner pops its list
    for (int r = 0; r < beam; r++) {
        float bv = top.v[0];
        int bi = top.i[0];
        block_argmax<NW>(r, bv, bi, redv, redi);
        top.retire(bi);
        if (tid == 0) sel_t[r] = bi;
    }
    __syncthreads();
    float* out = ws + (size_t)row * gb_row_floats(beam);
    if (tid == 0) {
        int cnt = 0;
        for (int r = 0; r < beam; r++) cnt += sel_t[r] != SEL_NONE ? 1 : 0;
        out[0] = p.m; out[1] = p.sum;
        reinterpret_cast<int*>(out)[2] = cnt;
    }
    if (tid < beam) reinterpret_cast<int*>(out)[GB_HDR + tid] = sel_t[tid];   // every entry is written: the kept tokens, best y first
}

// Stage 2 runs in fp64.  It handles at most beam^2 candidates per sample, so the cost is nothing; and fp32 is not enough for it: y = x + n
// carries ~3e-6 of rounding in fp32 (the noise's two logf, the temperature product, the sum), delta = Y - y inherits it, and
// log(1 - exp(-delta)) amplifies it by 1 / delta (measured with an fp32 stage 2 on an MI355X: 4.9e-5 in Gamma at beam 6, V = 4099, and
// 8.3e-6 in phi after five steps at V = 50257).  So the kept candidates' noise is drawn again from the same bits in fp64, x, lp, y, delta
// and the transform are fp64, and phi_c and Gamma_c are rounded to the fp32 state once.  Stage 1 keeps fp32: it only orders.
__device__ __forceinline__ double gumbel_of_bits_f64(uint32_t h) {
    const double e = h < 0x80000000u ? -log(((double)h + 0.5) * 0x1p-32) : -log1p(-(((double)(0xffffffffu - h) + 0.5) * 0x1p-32));
    return -log(e);
}
// log(1 - exp(-d)) for d > 0, each half through the function that is exact there
__device__ __forceinline__ double log1mexp(double d) { return d <= 0.6931471805599453 ? log(-expm1(-d)) : log1p(-exp(-d)); }

__global__ __launch_bounds__(64) void k_gumbel_final(const float* __restrict__ logits, size_t ldl, int beam, int V, float temp, int first,
                                                     int stop_token, uint64_t seed, int step, const float* __restrict__ ws,
                                                     float* __restrict__ scores, float* __restrict__ gumbels, float* __restrict__ seq_len,
                                                     unsigned char* __restrict__ stopped, int* __restrict__ next_tok, int* __restrict__ src_row) {
    __shared__ float red[2];
    __shared__ int redi[2];
    __shared__ double cy[GB_MAX * GB_MAX], clp[GB_MAX * GB_MAX], cn[GB_MAX * GB_MAX];
    __shared__ float cval[GB_MAX * GB_MAX], cphi[GB_MAX * GB_MAX];
    __shared__ int cidx[GB_MAX * GB_MAX], cflat[GB_MAX * GB_MAX];
    __shared__ float s_phi[GB_MAX], s_gam[GB_MAX], s_len[GB_MAX];
    __shared__ int s_st[GB_MAX], s_cnt[GB_MAX];
    __shared__ float sel_v[GB_MAX];
    __shared__ int sel_i[GB_MAX];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int nrows = first ? 1 : beam;
    // the parents' state, read before any slot is written; a stopped parent's workspace row was not written and is not read
    if (tid < beam) {
        const int r = s * beam + tid;
        const int st = first ? 0 : stopped[r];
        s_st[tid] = st;
        s_phi[tid] = first ? 0.f : scores[r];
        s_gam[tid] = first ? 0.f : gumbels[r];
        s_len[tid] = first ? 1.f : seq_len[r] + (st ? 0.f : 1.f);
        s_cnt[tid] = (st || tid >= nrows) ? 0 : min(max(reinterpret_cast<const int*>(ws + (size_t)r * gb_row_floats(beam))[2], 0), beam);
    }
    __syncthreads();
    const int ncand = nrows * beam;
    // pass 1: the kept candidates' x, lp, noise and y in fp64
    for (int c = tid; c < ncand; c += 64) {
        const int b = c / beam, j = c - b * beam;
        cflat[c] = SEL_NONE;
        if (j < s_cnt[b]) {
            const int row = s * beam + b;
            const float* rw = ws + (size_t)row * gb_row_floats(beam);
            const int v = min(max(reinterpret_cast<const int*>(rw)[GB_HDR + j], 0), V - 1);       // written by k_gumbel_rows: in [0, V)
            const double x = (double)logits[(size_t)row * ldl + v] / (double)temp;
            const double n = gumbel_of_bits_f64(philox_word(gumbel_bits4(seed, (uint32_t)step, (uint32_t)row, (uint32_t)(v >> 2)), (uint32_t)v & 3u));
            clp[c] = (x - (double)rw[0]) - log((double)rw[1]);       // log_softmax from the row's (max, sum of exp(x - max))
            cn[c] = n;
            cy[c] = x + n;
            cflat[c] = b * V + v;
        }
    }
    __syncthreads();
    // pass 2: the conditioned values
    for (int c = tid; c < ncand; c += 64) {
        const int b = c / beam, j = c - b * beam;
        float gc = -INFINITY, phic = -INFINITY;
        int flat = SEL_NONE;
        if (s_st[b]) {                                                  // a stopped parent continues with its padding token, unperturbed
            if (j == 0) { gc = s_gam[b]; phic = s_phi[b]; flat = b * V; }
        } else if (j < s_cnt[b]) {
            double Y = cy[b * beam];
            for (int q = 1; q < s_cnt[b]; q++) Y = fmax(Y, cy[b * beam + q]);
            const double gb = (double)s_gam[b], pc = (double)s_phi[b] + clp[c];
            const double d = Y - cy[c];                                 // >= 0; 0 for the row's best child
            if (d > 0.0) {
                const double t = gb - (pc + cn[c]) + log1mexp(d);
                gc = (float)(gb - fmax(0.0, t) - log1p(exp(-fabs(t))));   // = -log(exp(-Gamma_b) - exp(-Z) + exp(-g)), stable
            } else {
                gc = s_gam[b];                                          // bit for bit
            }
            phic = (float)pc;
            flat = cflat[c];
        }
        const bool ok = gc > -INFINITY;                                 // -inf (and NaN) is no candidate
        cval[c] = ok ? gc : -INFINITY;
        cphi[c] = phic;
        cidx[c] = ok ? flat : SEL_NONE;
    }
    __syncthreads();
    for (int c = tid; c < ncand; c += 64) cflat[c] = cidx[c];           // pick_from_list retires entries of cidx: the lookup below keeps a copy
    __syncthreads();
    pick_from_list<64>(cval, cidx, ncand, beam, red, redi, sel_v, sel_i);
    if (tid < beam) {
        const int o = s * beam + tid;
        const int idx = sel_i[tid];
        if (idx == SEL_NONE) {                                          // fewer candidates than slots: an empty slot, which stays empty
            next_tok[o] = 0;
            src_row[o] = 0;
            scores[o] = -INFINITY;
            gumbels[o] = -INFINITY;
            seq_len[o] = first ? 1.f : s_len[0] - (s_st[0] ? 0.f : 1.f);    // row 0's length as a stopped parent passes it on
            stopped[o] = 1;
        } else {
            const int b = idx / V, v = idx - b * V;                     // b < nrows by construction
            float phi = -INFINITY;
            for (int c = 0; c < ncand; c++)
                if (cflat[c] == idx) phi = cphi[c];
            next_tok[o] = v;
            src_row[o] = b;
            scores[o] = phi;
            gumbels[o] = sel_v[tid];
            seq_len[o] = s_len[b];
            stopped[o] = (unsigned char)(s_st[b] | (v == stop_token ? 1 : 0));
        }
    }
}

__global__ __launch_bounds__(256) void k_gumbel_noise(uint64_t seed, int step, int row, int V, float* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (4 * q >= V) return;
    const philox4 h = gumbel_bits4(seed, (uint32_t)step, (uint32_t)row, (uint32_t)q);
    for (int k = 0; k < 4; k++)
        if (4 * q + k < V) out[4 * q + k] = gumbel_of_bits(h.w[k]);
}

__global__ __launch_bounds__(256) void k_gumbel_from_bits(const uint32_t* __restrict__ h, int n, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = gumbel_of_bits(h[i]);
}

template <int K>
void launch_rows(hipStream_t st, int blocks, const float* logits, int64_t ldl, int beam, int V, float inv_temp, int first, uint64_t seed, int step,
                 const uint8_t* stopped, float* ws) {
    if ((ldl & 3) || ((uintptr_t)logits & 15))
        hipLaunchKernelGGL((k_gumbel_rows<K, false>), dim3(blocks), dim3(GR_T), 0, st, logits, (size_t)ldl, beam, V, inv_temp, first, seed, step, stopped, ws);
    else
        hipLaunchKernelGGL((k_gumbel_rows<K, true>), dim3(blocks), dim3(GR_T), 0, st, logits, (size_t)ldl, beam, V, inv_temp, first, seed, step, stopped, ws);
}

}  // namespace

extern "C" {

int64_t CC_API(cc_beam_gumbel_ws_bytes)(int32_t S, int32_t beam, int32_t V) {
    if (S < 0 || beam < 1 || beam > GB_MAX || V < 1) return CC_ERR_ARG;
    if (V > GB_VMAX) return CC_ERR_SHAPE;
    return (int64_t)S * beam * (int64_t)gb_row_floats(beam) * (int64_t)sizeof(float) + 512;
}

int CC_API(cc_beam_gumbel_step)(int32_t S, int32_t beam, int32_t V, const float* logits, int64_t ldl, float temperature, int32_t first,
                                int32_t stop_token, uint64_t seed, int32_t step, float* scores, float* gumbels, float* seq_lengths,
                                uint8_t* has_stopped, int32_t* next_tokens, int32_t* src_rows, void* ws, void* stream) {
    if (S < 0 || beam < 1 || beam > GB_MAX || V < 1 || ldl < V || step < 0 || temperature != temperature || !logits || !scores || !gumbels ||
        !seq_lengths || !has_stopped || !next_tokens || !src_rows || !ws)
        return CC_ERR_ARG;
    if (V > GB_VMAX) return CC_ERR_SHAPE;
    if (S == 0) return CC_OK;
    hipStream_t st = S_(stream);
    const float temp = temperature > 0.f ? temperature : 1.0f, inv_temp = 1.0f / temp;
    float* w = static_cast<float*>(ws);
    const int blocks = first ? S : S * beam;
    switch (beam) {
        case 1: launch_rows<1>(st, blocks, logits, ldl, beam, V, inv_temp, first, seed, step, has_stopped, w); break;
        case 2: launch_rows<2>(st, blocks, logits, ldl, beam, V, inv_temp, first, seed, step, has_stopped, w); break;
        case 3: launch_rows<3>(st, blocks, logits, ldl, beam, V, inv_temp, first, seed, step, has_stopped, w); break;
        case 4: launch_rows<4>(st, blocks, logits, ldl, beam, V, inv_temp, first, seed, step, has_stopped, w); break;
        case 5: launch_rows<5>(st, blocks, logits, ldl, beam, V, inv_temp, first, seed, step, has_stopped, w); break;
        case 8: launch_rows<8>(st, blocks, logits, ldl, beam, V, inv_temp, first, seed, step, has_stopped, w); break;
        default: launch_rows<GB_MAX>(st, blocks, logits, ldl, beam, V, inv_temp, first, seed, step, has_stopped, w); break;   // 6, 7, 9 .. 16
    }
    hipLaunchKernelGGL(k_gumbel_final, dim3(S), dim3(64), 0, st, logits, (size_t)ldl, beam, V, temp, first, stop_token, seed, step, w, scores, gumbels,
                       seq_lengths, has_stopped, next_tokens, src_rows);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int CC_API(cc_gumbel_noise)(uint64_t seed, int32_t step, int32_t row, int32_t V, float* out, void* stream) {
    if (step < 0 || row < 0 || V < 1 || !out) return CC_ERR_ARG;
    hipLaunchKernelGGL(k_gumbel_noise, dim3(((V + 3) / 4 + 255) / 256), dim3(256), 0, S_(stream), seed, step, row, V, out);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int CC_API(cc_gumbel_from_bits)(const uint32_t* h, int32_t n, float* out, void* stream) {
    if (n < 0 || !h || !out) return CC_ERR_ARG;
    if (n == 0) return CC_OK;
    hipLaunchKernelGGL(k_gumbel_from_bits, dim3((n + 255) / 256), dim3(256), 0, S_(stream), h, n, out);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // extern "C"
