// Label smoothing of the fused lm_head loss for gfx950, as rank-one corrections around the plain chain (kernels.h): the column mean wbar
// of wte's real rows, the rows' mean logit zbar = hf . wbar and loss term, the input-gradient update d hf += c (wte[t] - wbar), and the
// broadcast half of the tied weight gradient.  Bandwidth-bound row and column passes: 16-byte loads, one wave per row or one workgroup
// per (64 columns x a row slice), wave reductions.  Every sum runs in one fixed order, no atomics.
#include "kernels.h"

namespace CC_NS {

// Partial column sums of X[r][0:N] over the row slice of blockIdx.y: part[slice][c] = sum over the slice's rows of f(r) X[r][c], with
// f(r) = -coef[2 r + 1] (COEF; rows whose coefficient is 0 are not read) or 1.  Thread (rl, cg) walks rows r0 + rl, r0 + rl + 32, ... of
// its 8 columns; the 32 row lanes are then added in lane order.
template <bool COEF>
__global__ __launch_bounds__(256) void k_smooth_colpart(const act_t* __restrict__ X, int ld, int M, int N, int rows_per_slice,
                                                        const float* __restrict__ coef, float* __restrict__ part) {
    __shared__ float red[32][65];
    const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;
    const int col = blockIdx.x * 64 + cg * 8;
    const int r0 = blockIdx.y * rows_per_slice, r1 = min(M, r0 + rows_per_slice);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col < N) {
        int r = r0 + rl;
        if (!COEF) {      // four rows' loads in flight, added in row order (the order of the loop below)
            for (; r + 96 < r1; r += 128) {
                float f0[8], f1[8], f2[8], f3[8];
                act_ld8(X + (size_t)r * ld + col, f0);
                act_ld8(X + (size_t)(r + 32) * ld + col, f1);
                act_ld8(X + (size_t)(r + 64) * ld + col, f2);
                act_ld8(X + (size_t)(r + 96) * ld + col, f3);
#pragma unroll
                for (int e = 0; e < 8; e++) acc[e] = (((acc[e] + f0[e]) + f1[e]) + f2[e]) + f3[e];
            }
        }
        for (; r < r1; r += 32) {
            float w = 1.f;
            if (COEF) {
                w = -coef[2 * (size_t)r + 1];
                if (w == 0.f) continue;
            }
            float f[8];
            act_ld8(X + (size_t)r * ld + col, f);
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] += COEF ? w * f[e] : f[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; e++) red[rl][cg * 8 + e] = acc[e];
    __syncthreads();
    if (threadIdx.x < 64) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 32; r++) s += red[r][threadIdx.x];
        const int c = blockIdx.x * 64 + threadIdx.x;
        if (c < N) part[(size_t)blockIdx.y * N + c] = s;
    }
}
// second stage of the column mean: wbar[c] = (sum of part[k][c] over the slices) / V.  Lane group g (of 16) of a column adds slices g, g + 16,
// ... in that order; the 16 group sums are then added in group order.
__global__ __launch_bounds__(1024) void k_smooth_wbar_finish(const float* __restrict__ part, int S, int D, int V, float* __restrict__ wbar) {
    __shared__ float red[16][64];
    const int t = threadIdx.x & 63, g = threadIdx.x >> 6, c = blockIdx.x * 64 + t;
    float acc = 0.f;
    if (c < D)
        for (int k = g; k < S; k += 16) acc += part[(size_t)k * D + c];
    red[g][t] = acc;
    __syncthreads();
    if (g == 0 && c < D) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 16; q++) s += red[q][t];
        wbar[c] = s / (float)V;
    }
}
int smooth_wbar(const act_t* wte, int V, int D, float* part, float* wbar, hipStream_t st) {
    if ((D & 7) || V <= 0) return CC_ERR_SHAPE;
    const int S = smooth_wbar_slices(V);
    const int rps = ((V + S - 1) / S + 31) / 32 * 32;
    const int slices = (V + rps - 1) / rps;          // <= S
    hipLaunchKernelGGL(k_smooth_colpart<false>, dim3((D + 63) / 64, slices), dim3(256), 0, st, wte, D, V, D, rps, nullptr, part);
    hipLaunchKernelGGL(k_smooth_wbar_finish, dim3((D + 63) / 64), dim3(1024), 0, st, part, slices, D, V, wbar);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

// one wave per row: zbar[row] = hf[row] . wbar, term[row] = kept ? eps (z_t - zbar) : 0;  WT: the kept rows' terms times rw[row] (row_factor)
template <bool WT>
__global__ __launch_bounds__(256) void k_smooth_rows(const act_t* __restrict__ hf, const float* __restrict__ wbar, int D,
                                                     const int* __restrict__ target, const float* __restrict__ tgt, float eps,
                                                     const float* __restrict__ rw, float* __restrict__ zbar, float* __restrict__ term, int M) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const act_t* h = hf + (size_t)row * D;
    float acc = 0.f;
    for (int d = lane * 8; d < D; d += 512) {
        float a[8];
        act_ld8(h + d, a);
        const float4 b0 = *reinterpret_cast<const float4*>(wbar + d), b1 = *reinterpret_cast<const float4*>(wbar + d + 4);
        const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int e = 0; e < 8; e++) acc += a[e] * b[e];
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        zbar[row] = acc;
        term[row] = row_factor<WT>(target[row], eps * (tgt[row] - acc), rw, row);
    }
}
// one block, the order of k_ce_stats: stats3[2] = the plain sum ce_rows left in stats3[0], stats3[0] = that + the sum of the rows' terms.
// WT: ce_rows left the weighted sum in stats3[0] and the plain one in stats3[2] already, which stays.
template <bool WT>
__global__ __launch_bounds__(1024) void k_smooth_stats(const float* __restrict__ term, float* __restrict__ stats3, int M) {
    __shared__ float sl[16];
    float a = 0.f;
    for (int i = threadIdx.x; i < M; i += 1024) a += term[i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) sl[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        float ta = 0.f;
        for (int w = 0; w < 16; w++) ta += sl[w];
        const float nll = stats3[0];
        if (!WT) stats3[2] = nll;
        stats3[0] = nll + ta;
    }
}
int smooth_rows(const act_t* hf, const float* wbar, int D, const int* target, const float* tgt, float eps, float* zbar, float* term,
                float* stats3, int M, hipStream_t st, const float* row_weight) {
    if (D & 7) return CC_ERR_SHAPE;
    if (row_weight) {
        if (M > 0) hipLaunchKernelGGL(k_smooth_rows<true>, dim3((M + 3) / 4), dim3(256), 0, st, hf, wbar, D, target, tgt, eps, row_weight, zbar, term, M);
        hipLaunchKernelGGL(k_smooth_stats<true>, dim3(1), dim3(1024), 0, st, term, stats3, std::max(M, 0));
    } else {
        if (M > 0) hipLaunchKernelGGL(k_smooth_rows<false>, dim3((M + 3) / 4), dim3(256), 0, st, hf, wbar, D, target, tgt, eps, nullptr, zbar, term, M);
        hipLaunchKernelGGL(k_smooth_stats<false>, dim3(1), dim3(1024), 0, st, term, stats3, std::max(M, 0));
    }
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

// coef[row] = {0, -c}: c = eps * loss_scale / max(denom, 1) on kept rows, 0 elsewhere — the {r, w} layout of lm_rowfac, so that
// scatter_rows' act form adds value(row) = fl(c hf[row]) and leaves the rows with c == 0 out.  WT: c times rw[row] (row_factor), of either sign
template <bool WT>
__global__ void k_smooth_coef(const int* __restrict__ target, const float* __restrict__ denom, const float* __restrict__ loss_scale, float eps,
                              const float* __restrict__ rw, float* __restrict__ coef, int M) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float inv = (loss_scale ? loss_scale[0] : 1.0f) / fmaxf(denom[0], 1.0f);
    coef[2 * i] = 0.f;
    coef[2 * i + 1] = row_factor<WT>(target[i], -(eps * inv), rw, i);
}
// dhf[row][:] += c (wte[target[row]][:] - wbar[:]) in the stored type; rows with c == 0 are not touched
__global__ __launch_bounds__(256) void k_smooth_dhf(act_t* __restrict__ dhf, const float* __restrict__ coef, const int* __restrict__ target,
                                                    const act_t* __restrict__ wte, const float* __restrict__ wbar, int D, int M) {
    const int d8n = D >> 3;
    const size_t total = (size_t)M * d8n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / d8n), c = (int)(i % d8n) * 8;
        const float w = -coef[2 * (size_t)row + 1];
        if (w == 0.f) continue;
        float v[8], b[8];
        act_ld8(dhf + (size_t)row * D + c, v);
        act_ld8(wte + (size_t)target[row] * D + c, b);
        const float4 m0 = *reinterpret_cast<const float4*>(wbar + c), m1 = *reinterpret_cast<const float4*>(wbar + c + 4);
        const float m[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] += w * (b[e] - m[e]);
        act_st8(dhf + (size_t)row * D + c, v);
    }
}
int smooth_dhf(act_t* dhf, const int* target, const float* denom, const float* loss_scale, float eps, const act_t* wte, const float* wbar,
               float* coef, int D, int M, hipStream_t st, const float* row_weight) {
    if (D & 7) return CC_ERR_SHAPE;
    if (M <= 0) return CC_OK;
    if (row_weight) hipLaunchKernelGGL(k_smooth_coef<true>, dim3((M + 255) / 256), dim3(256), 0, st, target, denom, loss_scale, eps, row_weight, coef, M);
    else hipLaunchKernelGGL(k_smooth_coef<false>, dim3((M + 255) / 256), dim3(256), 0, st, target, denom, loss_scale, eps, nullptr, coef, M);
    hipLaunchKernelGGL(k_smooth_dhf, flat_grid((size_t)M * (D >> 3), 256, 4096), dim3(256), 0, st, dhf, coef, target, wte, wbar, D, M);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

// dwte[v][:] -= hsum[:] / V for the real rows v < V
__global__ __launch_bounds__(256) void k_smooth_bcast(float* __restrict__ dwte, const float* __restrict__ hsum, int D, int V) {
    const int d4n = D >> 2;
    const size_t total = (size_t)V * d4n;
    const float fv = (float)V;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % d4n) * 4;
        const float4 h = *reinterpret_cast<const float4*>(hsum + c);
        float4* p = reinterpret_cast<float4*>(dwte) + i;
        float4 g = *p;
        g.x -= h.x / fv; g.y -= h.y / fv; g.z -= h.z / fv; g.w -= h.w / fv;
        *p = g;
    }
}
// mode 2, the part of d wte that is not a row scatter: hsum = sum over kept rows of c hf (slice partials in the call's reduction scratch,
// folded in fold_partials' fixed order), then the broadcast subtraction over the V real rows of dwte
int smooth_dwte_bcast(const act_t* hf, const float* coef, int D, int M, int V, float* hsum, float* dwte, Call& cx) {
    const hipStream_t st = cx.st;
    if (D & 7) return CC_ERR_SHAPE;
    if (M <= 0) return CC_OK;
    const int S = std::min((M + 63) / 64, 256);
    const int rps = ((M + S - 1) / S + 31) / 32 * 32;
    const int slices = (M + rps - 1) / rps;
    float* part = red_scratch(cx, (size_t)slices * D);
    if (!part) return CC_ERR_STATE;
    if (hipMemsetAsync(hsum, 0, (size_t)D * sizeof(float), st) != hipSuccess) return CC_ERR_LAUNCH;
    hipLaunchKernelGGL(k_smooth_colpart<true>, dim3((D + 63) / 64, slices), dim3(256), 0, st, hf, D, M, D, rps, coef, part);
    FoldOut o{};
    o.p[0] = hsum; o.m = D; o.k = 1;
    const int rc = fold_partials(part, slices, D, 1, o, st);
    if (rc != CC_OK) return rc;
    hipLaunchKernelGGL(k_smooth_bcast, flat_grid((size_t)V * (D >> 2), 256, 8192), dim3(256), 0, st, dwte, hsum, D, V);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // namespace CC_NS
