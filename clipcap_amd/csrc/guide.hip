// Classifier-free guidance at decode time: one step's logits of the conditional stream (the language model behind the image prefix) and of
// the unconditional stream (the same tokens without it) combined into the guided scores the beam update (beam.hip) or the sampler
// (sample.hip) then reads (include/clipcap_hip.h cc_logits_guide):
//     out_i = scale * (c_i - lse_c) + (1 - scale) * (u_i - lse_u)          lse = log-sum-exp over the row's V real columns
// (Kornblith et al., ICCV 2023; Sanchez et al., 2023).  From outside this is two log_softmax passes and a lerp over [R][V] fp32 with two
// temporaries of that size; here it is one launch that reads both rows twice (the second time from L2 / the Infinity Cache) and writes one.
// fp32 work only, so this unit is built once (Makefile).
#include "layout.h"

using namespace CC_NS;

namespace {

constexpr int GD_T = 1024;                // threads per row (16 waves)
constexpr int GD_W = GD_T / 64;
constexpr int GD_VMAX = 1 << 30;          // element indices, rounded up to whole groups of 4 and one unrolled round, stay inside an int

// Elements are dealt out in groups of 4 consecutive columns: thread t owns groups t, t + GD_T, ... in BOTH passes and on BOTH paths.  VEC:
// a whole group (i + 4 <= V) moves as one 16-byte access; otherwise, and for the row's last partial group always, as scalars — the
// columns [V, ld) are never touched.  What a thread computes does not depend on the path, only how the bytes travel.
template <bool VEC>
__device__ __forceinline__ float4 gd_load(const float* row, int i, int V) {
    if (VEC && i + 4 <= V) return *reinterpret_cast<const float4*>(row + i);
    float4 r;
    r.x = i < V ? row[i] : -INFINITY;
    r.y = i + 1 < V ? row[i + 1] : -INFINITY;
    r.z = i + 2 < V ? row[i + 2] : -INFINITY;
    r.w = i + 3 < V ? row[i + 3] : -INFINITY;
    return r;
}
template <bool VEC>
__device__ __forceinline__ void gd_store(float* row, int i, int V, float4 v) {
    if (VEC && i + 4 <= V) { *reinterpret_cast<float4*>(row + i) = v; return; }
    if (i < V) row[i] = v.x;
    if (i + 1 < V) row[i + 1] = v.y;
    if (i + 2 < V) row[i + 2] = v.z;
    if (i + 3 < V) row[i + 3] = v.w;
}

// Running (max, sum of exp(x - max)) of one stream.  Eight elements share one rescale.  -inf entries (token bans, columns past V) add
// exactly 0; while nothing finite has been seen the reference point is 0, so that no -inf - -inf is formed.
struct GdAcc {
    float m = -INFINITY, s = 0.f;
    __device__ __forceinline__ void add(float4 a, float4 b) {
        const float bm = fmaxf(fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)), fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w)));
        const float mn = fmaxf(m, bm);
        const float ref = mn > -INFINITY ? mn : 0.f;
        const float ea = (__expf(a.x - ref) + __expf(a.y - ref)) + (__expf(a.z - ref) + __expf(a.w - ref));
        const float eb = (__expf(b.x - ref) + __expf(b.y - ref)) + (__expf(b.z - ref) + __expf(b.w - ref));
        s = fmaf(s, __expf(m - ref), ea + eb);
        m = mn;
    }
};

// log-sum-exp of the row from the threads' running pairs: wave by DPP (common.hip.h), then the GD_W wave results in index order from
// LDS.  Every thread of the block calls it and gets the same value; -inf for a row without a finite entry.
__device__ __forceinline__ float gd_block_lse(GdAcc a, float* red_m, float* red_s) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float wm = wave_max(a.m);
    const float wref = wm > -INFINITY ? wm : 0.f;
    const float ws = wave_sum(a.s * __expf(a.m - wref));
    if (lane == 0) { red_m[wv] = wm; red_s[wv] = ws; }
    __syncthreads();
    float M = red_m[0];
#pragma unroll
    for (int w = 1; w < GD_W; w++) M = fmaxf(M, red_m[w]);
    if (!(M > -INFINITY)) return -INFINITY;
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < GD_W; w++) S += red_s[w] * __expf(red_m[w] - M);
    return M + logf(S);
}

__device__ __forceinline__ float gd_mix(float c, float u, float lc, float lu, float scale, float oms) {
    // a token banned in either stream stays banned; with both finite, both lse are finite too
    return (c == -INFINITY || u == -INFINITY) ? -INFINITY : fmaf(scale, c - lc, oms * (u - lu));
}

// One workgroup owns one row.  Pass 1: one sweep over both streams, two groups of each in flight per thread.  Pass 2: the same sweep
// again (the two rows are 2 * V * 4 bytes, just read: they come back from L2 / the Infinity Cache) and the store.  In place (out == cond)
// is safe because a thread reads in pass 2 exactly the elements it writes, and pass 1 is over for the whole block (the barrier inside
// gd_block_lse) before the first store.
template <bool VEC>
__global__ __launch_bounds__(GD_T) void k_logits_guide(const float* cond, size_t ld_c, const float* uncond, size_t ld_u, int V, float scale, float* out,
                                                       size_t ld_o, const unsigned char* __restrict__ skip) {
    __shared__ float red[4][GD_W];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (skip && skip[row]) return;                                      // block-uniform, before any barrier or wave reduction
    const float* cr = cond + (size_t)row * ld_c;
    const float* ur = uncond + (size_t)row * ld_u;
    float* orow = out + (size_t)row * ld_o;
    const int ng = (V + 3) >> 2;
    GdAcc ac, au;
    for (int g0 = tid; g0 < ng; g0 += 2 * GD_T) {
        const int i0 = g0 * 4, i1 = (g0 + GD_T) * 4;                    // i1 may lie past the row: such a group is all -inf and loads nothing
        const float4 c0 = gd_load<VEC>(cr, i0, V), u0 = gd_load<VEC>(ur, i0, V);
        const float4 c1 = gd_load<VEC>(cr, i1, V), u1 = gd_load<VEC>(ur, i1, V);
        ac.add(c0, c1);
        au.add(u0, u1);
    }
    const float lc = gd_block_lse(ac, red[0], red[1]);
    const float lu = gd_block_lse(au, red[2], red[3]);
    const float oms = 1.0f - scale;
    for (int g0 = tid; g0 < ng; g0 += 2 * GD_T) {
        const int i0 = g0 * 4, i1 = (g0 + GD_T) * 4;
        const float4 c0 = gd_load<VEC>(cr, i0, V), u0 = gd_load<VEC>(ur, i0, V);
        const float4 c1 = gd_load<VEC>(cr, i1, V), u1 = gd_load<VEC>(ur, i1, V);
        float4 o0, o1;
        o0.x = gd_mix(c0.x, u0.x, lc, lu, scale, oms); o0.y = gd_mix(c0.y, u0.y, lc, lu, scale, oms);
        o0.z = gd_mix(c0.z, u0.z, lc, lu, scale, oms); o0.w = gd_mix(c0.w, u0.w, lc, lu, scale, oms);
        o1.x = gd_mix(c1.x, u1.x, lc, lu, scale, oms); o1.y = gd_mix(c1.y, u1.y, lc, lu, scale, oms);
        o1.z = gd_mix(c1.z, u1.z, lc, lu, scale, oms); o1.w = gd_mix(c1.w, u1.w, lc, lu, scale, oms);
        gd_store<VEC>(orow, i0, V, o0);
        gd_store<VEC>(orow, i1, V, o1);
    }
}

}  // namespace

extern "C" {

int CC_API(cc_logits_guide)(const float* cond, int64_t ld_c, const float* uncond, int64_t ld_u, int32_t R, int32_t V, float scale, float* out,
                            int64_t ld_o, const uint8_t* skip_rows, void* stream) {
    if (!out) { out = const_cast<float*>(cond); ld_o = ld_c; }          // in place
    if (R < 0 || V <= 0 || ld_c < V || ld_u < V || ld_o < V || !__builtin_isfinite(scale) || scale < 0.f) return CC_ERR_ARG;
    if (R == 0) return CC_OK;
    if (!cond || !uncond) return CC_ERR_ARG;
    if (V > GD_VMAX) return CC_ERR_SHAPE;
    const bool vec = (((uintptr_t)cond | (uintptr_t)uncond | (uintptr_t)out) & 15) == 0 && ((ld_c | ld_u | ld_o) & 3) == 0;
    hipStream_t st = S_(stream);
    if (vec)
        hipLaunchKernelGGL(k_logits_guide<true>, dim3(R), dim3(GD_T), 0, st, cond, (size_t)ld_c, uncond, (size_t)ld_u, V, scale, out, (size_t)ld_o,
                           skip_rows);
    else
        hipLaunchKernelGGL(k_logits_guide<false>, dim3(R), dim3(GD_T), 0, st, cond, (size_t)ld_c, uncond, (size_t)ld_u, V, scale, out, (size_t)ld_o,
                           skip_rows);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // extern "C"
