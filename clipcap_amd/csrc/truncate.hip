// Truncation rules for the sampling decoders, in front of the sampling step (sample.hip): min-p (Nguyen et al., 2024), the epsilon and eta
// cutoffs (Hewitt et al., 2022) and locally typical sampling (Meister et al., 2022) on one step's logits, in place: the raw logit of every
// removed token becomes -inf, every kept logit stays bit-untouched (include/clipcap_hip.h cc_logits_truncate).  The rules act on the
// values the sampler draws from, v_i = fl32(pen(x_i) * fl32(1 / T)) — SmRow::xform of sample.hip, restated here because that file's results
// are pinned bit for bit and stay untouched; tests/sample_ref.row_values is the one statement both are held to.
// One workgroup per row, one launch.  The row (V = 50257: 200 KB) does not fit LDS and is re-read from L2 per pass, TR_U loads in flight
// per thread (sample.hip records why).  Passes: maximum / smallest finite value; the two sums that give lse and the entropy H (only with
// epsilon, eta or typical on); for typical a weighted threshold search over d = |lse - H - v| ascending — one pass into TR_NB linear buckets of
// d, three exact radix passes (11/11/10 bits of d's fp32 image) inside the crossing bucket, masses in 2^-32 fixed point: integer atomics
// only, so the order of arrival does not matter; one pass for the empty-intersection test (only with typical AND a threshold rule on);
// the pass that writes the -inf.  The three threshold rules fold into one scalar threshold on v.
// No operand-dependent work, so this unit is built once (Makefile); the few row statistics (two sums, lse, H, the thresholds) are held in
// fp64 so that their error is that of __expf alone (tests/truncate_ref.py counts it).
#include "layout.h"

using namespace CC_NS;

namespace {

constexpr int TR_T = 1024;                  // threads per row
constexpr int TR_W = TR_T / 64;
constexpr int TR_NB = 2048;                 // buckets of a selection pass
constexpr int TR_U = 8;                     // loads in flight per thread
constexpr size_t TR_LDS_MAX = 150 * 1024;
constexpr unsigned TR_NONE = 0xffffffffu;
enum { TR_MINP = 1, TR_EPS = 2, TR_ETA = 4, TR_TYP = 8 };

struct TrRow {
    float* x;
    const unsigned* bitmap;   // LDS: history tokens (repetition penalty)
    float rep_pen, inv_temp;
    bool use_rep;
    __device__ __forceinline__ float val(int i, float v) const {
        if (use_rep && ((bitmap[i >> 5] >> (i & 31)) & 1u)) v = v < 0.f ? v * rep_pen : v / rep_pen;   // penalty first, then temperature
        float t = v * inv_temp;
        asm volatile("" : "+v"(t));      // the ROUNDED product is the value in every pass: nothing downstream may fuse with this multiply
        return t;
    }
};

template <class F>
__device__ __forceinline__ void tr_sweep(const TrRow& r, int V, F f) {      // f(i, raw logit, value)
    for (int i0 = threadIdx.x; i0 < V; i0 += TR_T * TR_U) {
        float raw[TR_U];
#pragma unroll
        for (int k = 0; k < TR_U; k++) { const int i = i0 + k * TR_T; raw[k] = i < V ? r.x[i] : 0.f; }
#pragma unroll
        for (int k = 0; k < TR_U; k++) { const int i = i0 + k * TR_T; if (i < V) f(i, raw[k], r.val(i, raw[k])); }
    }
}

// distance of a value from the centre c = lse - H, rounded to fp32 ONCE: the same number in every pass (its bits are the selection key:
// d >= 0, so larger d <-> larger key; -inf gives +inf)
__device__ __forceinline__ float tr_d(double c, float v) {
    float d = (float)fabs(c - (double)v);
    asm volatile("" : "+v"(d));
    return d;
}
__device__ __forceinline__ int tr_lb(float d, float dscale) { return (int)fminf(d * dscale, (float)(TR_NB - 1)); }
// 2^-32 fixed point: exp(v - m) <= 1 scaled to just under 2^32 (4294967040 = the largest float below 2^32), as the sampler's masses
__device__ __forceinline__ unsigned long long tr_w(float v, float m) { return (unsigned long long)(unsigned)(__expf(v - m) * 4294967040.0f); }

// exclusive prefix sum over the block in thread order; *total gets the block sum.  red: [TR_W]
__device__ __forceinline__ unsigned long long tr_block_excl(unsigned long long v, unsigned long long* red, unsigned long long* total) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    unsigned long long inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long n = __shfl_up(inc, o, 64);
        if (l >= o) inc += n;
    }
    __syncthreads();
    if (l == 63) red[w] = inc;
    __syncthreads();
    unsigned long long base = 0, t = 0;
    for (int i = 0; i < TR_W; i++) {
        if (i < w) base += red[i];
        t += red[i];
    }
    *total = t;
    return base + inc - v;
}

// Key of d*: the smallest key K with (mass of the finite elements whose key <= K) >= trunc(typical_p * total mass).  Thread t owns
// buckets 2t and 2t + 1 of a pass; `acc` = the mass strictly below the bucket chosen so far.  TR_NONE = keep everything (cannot happen
// while the passes agree on every element's bucket; kept as the safe answer).
__device__ unsigned tr_select(const TrRow& r, int V, float m, double c, float dscale, float typical_p, unsigned long long* hist_w,
                              unsigned long long* red, unsigned* bcast) {
    const int b0 = 2 * (int)threadIdx.x, b1 = b0 + 1;
    for (int b = threadIdx.x; b < TR_NB; b += TR_T) hist_w[b] = 0;
    __syncthreads();
    tr_sweep(r, V, [&](int, float, float v) {
        if (v > -INFINITY) atomicAdd(&hist_w[tr_lb(tr_d(c, v), dscale)], tr_w(v, m));
    });
    __syncthreads();
    unsigned long long w0 = hist_w[b0], w1 = hist_w[b1], tot;
    unsigned long long before = tr_block_excl(w0 + w1, red, &tot);
    unsigned long long target = (unsigned long long)((double)typical_p * (double)tot);
    if (target == 0) target = 1;                                // the closest token is always kept
    if (threadIdx.x == 0) bcast[0] = TR_NONE;
    __syncthreads();
    if (before < target && before + w0 + w1 >= target) {
        const bool first = before + w0 >= target;
        bcast[0] = (unsigned)(first ? b0 : b1);
        red[TR_W] = before + (first ? 0 : w0);
    }
    __syncthreads();
    if (bcast[0] == TR_NONE) return TR_NONE;
    const int lbsel = (int)bcast[0];
    unsigned long long acc = red[TR_W];
    __syncthreads();
    unsigned prefix = 0, mask = 0;
    const int shifts[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
    for (int pass = 0; pass < 3; pass++) {
        const int sh = shifts[pass], nb = 1 << bits[pass];
        for (int b = threadIdx.x; b < TR_NB; b += TR_T) hist_w[b] = 0;
        __syncthreads();
        tr_sweep(r, V, [&](int, float, float v) {
            if (!(v > -INFINITY)) return;
            const float d = tr_d(c, v);
            const unsigned k = __float_as_uint(d);
            if (tr_lb(d, dscale) == lbsel && (k & mask) == prefix) atomicAdd(&hist_w[(k >> sh) & (nb - 1)], tr_w(v, m));
        });
        __syncthreads();
        w0 = b0 < nb ? hist_w[b0] : 0;
        w1 = b1 < nb ? hist_w[b1] : 0;
        before = acc + tr_block_excl(w0 + w1, red, &tot);
        if (threadIdx.x == 0) bcast[0] = TR_NONE;
        __syncthreads();
        if (before < target && before + w0 + w1 >= target) {
            const bool first = before + w0 >= target;
            bcast[0] = (unsigned)(first ? b0 : b1);
            red[TR_W] = before + (first ? 0 : w0);
        }
        __syncthreads();
        if (bcast[0] == TR_NONE) return TR_NONE;
        acc = red[TR_W];
        prefix |= bcast[0] << sh;
        mask |= (unsigned)(nb - 1) << sh;
        __syncthreads();
    }
    return prefix;
}

__global__ __launch_bounds__(TR_T) void k_logits_truncate(float* logits, size_t ld, int V, float inv_temp, const long long* __restrict__ hist,
                                                          int hist_len, int hist_ld, float rep_pen, int rules, double ln_minp, double ln_eps,
                                                          double ln_eta, float typical_p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_raw[];
    unsigned long long* hist_w = reinterpret_cast<unsigned long long*>(tr_raw);                 // [TR_NB]
    unsigned long long* red = hist_w + TR_NB;                                                   // [TR_W + 2]
    double* dred = reinterpret_cast<double*>(red + TR_W + 2);                                   // [2 TR_W]
    float* fred = reinterpret_cast<float*>(dred + 2 * TR_W);                                    // [2 TR_W]
    unsigned* bcast = reinterpret_cast<unsigned*>(fred + 2 * TR_W);                             // [4]
    unsigned* bitmap = bcast + 4;                                                               // [(V + 31) / 32]
    const int row = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    TrRow r;
    r.x = logits + (size_t)row * ld;
    r.bitmap = bitmap;
    r.rep_pen = rep_pen;
    r.inv_temp = inv_temp;
    r.use_rep = hist != nullptr && hist_len > 0 && rep_pen != 1.0f;
    if (r.use_rep) {
        for (int i = threadIdx.x; i < (V + 31) / 32; i += TR_T) bitmap[i] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < hist_len; i += TR_T) {
            const long long t = hist[(size_t)row * hist_ld + i];
            if (t >= 0 && t < V) atomicOr(&bitmap[t >> 5], 1u << (t & 31));
        }
        __syncthreads();
    }
    // row maximum and smallest finite value
    float m = -INFINITY, mn = INFINITY;
    tr_sweep(r, V, [&](int, float, float v) {
        m = fmaxf(m, v);
        if (v > -INFINITY) mn = fminf(mn, v);
    });
    for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o, 64)); mn = fminf(mn, __shfl_xor(mn, o, 64)); }
    if (lane == 0) { fred[wave] = m; fred[TR_W + wave] = mn; }
    __syncthreads();
    m = fred[0]; mn = fred[TR_W];
    for (int i = 1; i < TR_W; i++) { m = fmaxf(m, fred[i]); mn = fminf(mn, fred[TR_W + i]); }
    if (!(m > -INFINITY)) return;                               // a row of only -inf is left as it is (block-uniform)
    // S0 = sum of e_i, S1 = sum of e_i (v_i - m), e_i = __expf(v_i - m): lse = m + log S0, H = log S0 - S1 / S0, centre lse - H = m + S1 / S0.
    // fp64 accumulators in a fixed order: thread-strided, the wave's butterfly, the waves in index order.
    double lse = 0.0, H = 0.0, centre = 0.0;
    if (rules & (TR_EPS | TR_ETA | TR_TYP)) {
        double s0 = 0.0, s1 = 0.0;
        tr_sweep(r, V, [&](int, float, float v) {
            const float xm = v - m, e = __expf(xm);
            if (e > 0.f) { s0 += (double)e; s1 += (double)e * (double)xm; }      // p_i > 0 only: no 0 * -inf
        });
        for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); }
        if (lane == 0) { dred[wave] = s0; dred[TR_W + wave] = s1; }
        __syncthreads();
        s0 = 0.0; s1 = 0.0;
        for (int i = 0; i < TR_W; i++) { s0 += dred[i]; s1 += dred[TR_W + i]; }
        const double ls = log(s0), q = s1 / s0;                 // s0 >= 1: the maximum's own term
        lse = (double)m + ls;
        H = ls - q;
        centre = (double)m + q;
    }
    // the threshold rules as one threshold on v: keep v >= thr; thr_f = the smallest fp32 >= thr, so the fp32 compare decides the same
    double thr = -INFINITY;
    if (rules & TR_MINP) thr = fmax(thr, (double)m + ln_minp);
    if (rules & TR_EPS) thr = fmax(thr, lse + ln_eps);
    if (rules & TR_ETA) thr = fmax(thr, lse + fmin(ln_eta, 0.5 * ln_eta - H));
    float thr_f = (float)thr;
    if ((double)thr_f < thr) thr_f = __uint_as_float(thr_f > 0.f ? __float_as_uint(thr_f) + 1u : thr_f < 0.f ? __float_as_uint(thr_f) - 1u : 1u);
    // typical: the key of d*
    const bool typ = (rules & TR_TYP) != 0;
    unsigned dkey = TR_NONE;
    if (typ) {
        const float dmax = fmaxf(tr_d(centre, m), tr_d(centre, mn));
        const float dscale = dmax > 0.f ? ((float)TR_NB - 0.001f) / dmax : 0.f;
        dkey = tr_select(r, V, m, centre, dscale, typical_p, hist_w, red, bcast);
    }
    auto kept = [=](float v) { return v >= thr_f && (!typ || __float_as_uint(tr_d(centre, v)) <= dkey); };
    // an empty intersection keeps the maxima.  The maximum passes a threshold rule if any token does; typical alone always keeps a token.
    bool empty = !(m >= thr_f);
    if (!empty && typ && (rules & (TR_MINP | TR_EPS | TR_ETA))) {
        int any = 0;
        tr_sweep(r, V, [&](int, float, float v) { any |= kept(v) ? 1 : 0; });
        empty = !__syncthreads_or(any);
    }
    tr_sweep(r, V, [&](int i, float raw, float v) {
        const bool k = empty ? v == m : kept(v);
        if (!k && raw != -INFINITY) r.x[i] = -INFINITY;
    });
}

size_t truncate_lds_bytes(int V) {
    return (size_t)TR_NB * 8 + (TR_W + 2) * 8 + 2 * TR_W * 8 + 2 * TR_W * 4 + 16 + (size_t)((V + 31) / 32) * 4;
}

}  // namespace

extern "C" {

int CC_API(cc_logits_truncate)(float* logits, int32_t R, int32_t V, int64_t ldl, float temperature, const int64_t* history, int32_t hist_len,
                               int32_t hist_ld, float repetition_penalty, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff,
                               void* stream) {
    if (R < 0 || V <= 0 || ldl < V) return CC_ERR_ARG;
    if (!(min_p >= 0.f && min_p <= 1.f) || !(typical_p > 0.f && typical_p <= 1.f) || !(epsilon_cutoff >= 0.f && epsilon_cutoff < 1.f) ||
        !(eta_cutoff >= 0.f && eta_cutoff < 1.f))
        return CC_ERR_ARG;                                      // NaN fails every comparison
    if (hist_len < 0 || (hist_len > 0 && (!history || hist_ld < hist_len))) return CC_ERR_ARG;
    if (R > 0 && !logits) return CC_ERR_ARG;
    const int rules = (min_p > 0.f ? TR_MINP : 0) | (epsilon_cutoff > 0.f ? TR_EPS : 0) | (eta_cutoff > 0.f ? TR_ETA : 0) | (typical_p < 1.f ? TR_TYP : 0);
    if (R == 0 || rules == 0) return CC_OK;                     // nothing to do: nothing is launched
    const size_t sh = truncate_lds_bytes(V);
    if (sh > TR_LDS_MAX) return CC_ERR_SHAPE;
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)k_logits_truncate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TR_LDS_MAX); attr = true; }
    const float inv_temp = temperature > 0.f ? 1.0f / temperature : 1.0f;          // as the sampling step takes it
    const double ln_minp = min_p > 0.f ? log((double)min_p) : 0.0, ln_eps = epsilon_cutoff > 0.f ? log((double)epsilon_cutoff) : 0.0,
                 ln_eta = eta_cutoff > 0.f ? log((double)eta_cutoff) : 0.0;
    hipLaunchKernelGGL(k_logits_truncate, dim3(R), dim3(TR_T), sh, S_(stream), logits, (size_t)ldl, V, inv_temp,
                       reinterpret_cast<const long long*>(history), hist_len, hist_ld, repetition_penalty, rules, ln_minp, ln_eps, ln_eta, typical_p);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // extern "C"
