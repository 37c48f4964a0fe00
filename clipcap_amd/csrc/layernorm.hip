// LayerNorm forward and backward for gfx950: one wave per row, the row cached in registers.  The backward's parameter gradients are
// folded by reduce.hip.
#include "kernels.h"

namespace CC_NS {

// ------------------------------------------------------------------------------------------------------------
// LayerNorm forward: one wave per row, row cached in registers (D <= 2048, D % 4 == 0).
// y(bf16)[r] = (x[map(r)] - mean) * rstd * gamma + beta ; saves mean / rstd per output row.
// ------------------------------------------------------------------------------------------------------------
constexpr int LN_MAXV = 8;  // float4 per lane -> D <= 2048
// D -> the NV instantiation, for both launchers: LAUNCH(NV, ...) with the smallest NV of 1, 2, 3, 4, LN_MAXV that has D <= 256 NV
#define LN_NV(D, LAUNCH, ...) { if ((D) <= 256) LAUNCH(1, ##__VA_ARGS__); else if ((D) <= 512) LAUNCH(2, ##__VA_ARGS__); else if ((D) <= 768) LAUNCH(3, ##__VA_ARGS__); else if ((D) <= 1024) LAUNCH(4, ##__VA_ARGS__); else LAUNCH(LN_MAXV, ##__VA_ARGS__); }
__device__ __forceinline__ int ln_col(int lane, int it) { return lane * 4 + it * 256; }      // first of the lane's 4 columns in its it-th float4

template <int NV>   // float4 per lane actually used: D <= 256 NV (a run-time bound of 8 kept 8 x 4 registers live per array)
__global__ __launch_bounds__(256) void k_ln_fwd(const float* __restrict__ x, int ldx, const int* __restrict__ row_map,
                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                act_t* __restrict__ y, float* __restrict__ y32, float* __restrict__ mean,
                                                float* __restrict__ rstd, int rows, int D, float eps, int img) {
    // img (bf16x3 build only): y receives the [hi | hi | lo] operand image of the consumer GEMM (rows of 3 D 16-bit elements) instead of
    // the fp32 activation — gemm.hip.h::epi_store8's layout and arithmetic, four elements at a time
    constexpr int R = NV <= 4 ? 2 : 1;       // rows per wave, loaded together: one row per wave is a chain of exposed round trips
    const int lane = threadIdx.x & 63;
    const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (row0 >= rows) return;
    float4 v[R][NV], g[NV], bt[NV];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int row = min(row0 + r, rows - 1);
        const float* xr = x + (size_t)(row_map ? row_map[row] : row) * ldx;
#pragma unroll
        for (int it = 0; it < NV; it++) {
            const int c = ln_col(lane, it);
            v[r][it] = c < D ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0, 0, 0, 0);
        }
    }
#pragma unroll
    for (int it = 0; it < NV; it++) {        // affine parameters fetched with the rows, not after the reductions
        const int c = ln_col(lane, it);
        g[it] = c < D ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(0, 0, 0, 0);
        bt[it] = c < D ? *reinterpret_cast<const float4*>(beta + c) : make_float4(0, 0, 0, 0);
    }
    float mu[R], rs[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        float s = 0.f;
#pragma unroll
        for (int it = 0; it < NV; it++) s += v[r][it].x + v[r][it].y + v[r][it].z + v[r][it].w;
        mu[r] = wave_sum(s) / D;
        float q = 0.f;
#pragma unroll
        for (int it = 0; it < NV; it++) {
            const int c = ln_col(lane, it);
            if (c < D) {
                const float a = v[r][it].x - mu[r], b = v[r][it].y - mu[r], cc_ = v[r][it].z - mu[r], d = v[r][it].w - mu[r];
                q += a * a + b * b + cc_ * cc_ + d * d;
            }
        }
        rs[r] = rsqrtf(wave_sum(q) / D + eps);
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int row = row0 + r;
        if (row >= rows) break;
        if (lane == 0) {
            if (mean) mean[row] = mu[r];
            if (rstd) rstd[row] = rs[r];
        }
#pragma unroll
        for (int it = 0; it < NV; it++) {
            const int c = lane * 4 + it * 256;      // ln_col, written out: through the function NV = 1 and 2 compile to other code here
            if (c < D) {
                const float o0 = (v[r][it].x - mu[r]) * rs[r] * g[it].x + bt[it].x, o1 = (v[r][it].y - mu[r]) * rs[r] * g[it].y + bt[it].y;
                const float o2 = (v[r][it].z - mu[r]) * rs[r] * g[it].z + bt[it].z, o3 = (v[r][it].w - mu[r]) * rs[r] * g[it].w + bt[it].w;
#if CC_OP == 2
                if (y && img) {
                    uint2 hi, lo;
                    x3_pair4(o0, o1, o2, o3, hi, lo);
                    op16_t* r3 = reinterpret_cast<op16_t*>(y) + (size_t)row * 3 * D + c;      // x3_store4, written out for the same reason
                    *reinterpret_cast<uint2*>(r3) = hi;
                    *reinterpret_cast<uint2*>(r3 + D) = hi;
                    *reinterpret_cast<uint2*>(r3 + 2 * D) = lo;
                } else
#endif
                if (y) act_st4(y + (size_t)row * D + c, o0, o1, o2, o3);
                if (y32) *reinterpret_cast<float4*>(y32 + (size_t)row * D + c) = make_float4(o0, o1, o2, o3);
            }
        }
    }
}
int ln_fwd(const float* x, int ldx, const int* row_map, const float* gamma, const float* beta, Act yo, float* y32,
           float* mean, float* rstd, int rows, int D, hipStream_t st) {
    if (D > LN_MAXV * 256 || (D & 3) || (ldx & 3)) return CC_ERR_SHAPE;
    if (rows <= 0) return CC_OK;
    const int rpb = D <= 1024 ? 8 : 4;      // rows per block: 4 waves x (2 rows for NV <= 4, else 1)
    const dim3 gr((rows + rpb - 1) / rpb);
    act_t* const y = yo.p;
    const int img = yo.img ? 1 : 0;           // y leaves as its consumer GEMM's operand image
    if (img && (!kX3 || yo.img != D)) return CC_ERR_STATE;
#define LN_FWD(NV) hipLaunchKernelGGL(k_ln_fwd<NV>, gr, dim3(256), 0, st, x, ldx, row_map, gamma, beta, y, y32, mean, rstd, rows, D, 1e-5f, img)
    LN_NV(D, LN_FWD)
#undef LN_FWD
    return CC_OK;
}

// LayerNorm backward.  dy(bf16)[r]; x[map(r)]; mean/rstd[r].  dx_out[map(r)] = (dres ? dres[map(r)] : 0) + dLN ; also a
// bf16 copy of dx_out for the next dgrad GEMM.  Optional dgamma/dbeta (one partial sum per column per block into `part`, folded
// in a fixed order by k_fold_partials) and, with them, dcol[c] += sum_r dx16[r][c] — the bias gradient of the Linear whose output gradient dx16 is
// (column sums of the 16-bit values, exactly what k_colsum_bf16 on dx16 gives): one launch less per bias.
// Each wave walks rows  row = blockIdx*4 + wave + k*gridDim*4.
template <int NV, bool DG, int NW>   // NV as in k_ln_fwd; DG: accumulate dgamma / dbeta; NW waves per block
__global__ __launch_bounds__(NW * 64) void k_ln_bwd(const act_t* __restrict__ dy, const float* __restrict__ x, int ldx,
                                                const int* __restrict__ row_map, const float* __restrict__ mean,
                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                const float* __restrict__ dres, float* __restrict__ dx32,
                                                act_t* __restrict__ dx16, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                float* __restrict__ dcol, int rows, int D, Drop dmask, int img, float* __restrict__ part) {
    // img (bf16x3 build, ldx == D): dx16 receives the [hi | hi | lo] operand image of the input-gradient GEMM that reads it
    extern __shared__ __attribute__((aligned(16))) float ln_red[];  // [2][NW][D] when dgamma
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4 pg[DG ? NV : 1], pb[DG ? NV : 1], pc[DG ? NV : 1];
#pragma unroll
    for (int it = 0; it < (DG ? NV : 1); it++) pg[it] = pb[it] = pc[it] = make_float4(0, 0, 0, 0);
    // the row loop is a chain of dependent HBM round trips when a wave owns several rows (the parameter-gradient form keeps the grid
    // at one block per CU): the next row's operands are requested before the current row is reduced
    float4 gmv[NV];
#pragma unroll
    for (int it = 0; it < NV; it++) {
        const int c = ln_col(lane, it);
        gmv[it] = c < D ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(0, 0, 0, 0);
    }
    struct RowIn { act_raw4 d[NV]; float4 xv[NV], rr[NV]; float mu, rs; size_t xr; };
    auto fetch = [&](int row, RowIn& r) {
        r.xr = (size_t)(row_map ? row_map[row] : row) * ldx;
        r.mu = mean[row]; r.rs = rstd[row];
#pragma unroll
        for (int it = 0; it < NV; it++) {
            const int c = ln_col(lane, it);
            if (c < D) {
                r.d[it] = act_ldraw4(dy + (size_t)row * D + c);
                r.xv[it] = *reinterpret_cast<const float4*>(x + r.xr + c);
                r.rr[it] = dres ? *reinterpret_cast<const float4*>(dres + r.xr + c) : make_float4(0, 0, 0, 0);
            }
        }
    };
    const int rstep = gridDim.x * NW;
    int row = blockIdx.x * NW + wave;
    RowIn cur;
    if (row < rows) fetch(row, cur);
    for (; row < rows; row += rstep) {
        RowIn nxt;
        const bool more = DG && row + rstep < rows;      // the plain form runs one row per wave (grid covers the rows): no second register set
        if constexpr (DG) { if (more) fetch(row + rstep, nxt); }
        const size_t xr = cur.xr;
        const float mu = cur.mu, rs = cur.rs;
        float4 g[NV], xh[NV], rr[NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int it = 0; it < NV; it++) {
            const int c = ln_col(lane, it);
            if (c < D) {
                float d0, d1, d2, d3;
                act_unpack4(cur.d[it], d0, d1, d2, d3);
                const float4 xv = cur.xv[it];
                const float4 gm = gmv[it];
                rr[it] = cur.rr[it];
                xh[it] = make_float4((xv.x - mu) * rs, (xv.y - mu) * rs, (xv.z - mu) * rs, (xv.w - mu) * rs);
                g[it] = make_float4(d0 * gm.x, d1 * gm.y, d2 * gm.z, d3 * gm.w);
                s1 += g[it].x + g[it].y + g[it].z + g[it].w;
                s2 += g[it].x * xh[it].x + g[it].y * xh[it].y + g[it].z * xh[it].z + g[it].w * xh[it].w;
                if constexpr (DG) {
                    pg[it].x += d0 * xh[it].x; pg[it].y += d1 * xh[it].y; pg[it].z += d2 * xh[it].z; pg[it].w += d3 * xh[it].w;
                    pb[it].x += d0; pb[it].y += d1; pb[it].z += d2; pb[it].w += d3;
                }
            }
        }
        const float m1 = wave_sum(s1) / D, m2 = wave_sum(s2) / D;
#pragma unroll
        for (int it = 0; it < NV; it++) {
            const int c = ln_col(lane, it);
            if (c < D) {
                float4 o = make_float4(rs * (g[it].x - m1 - xh[it].x * m2), rs * (g[it].y - m1 - xh[it].y * m2),
                                       rs * (g[it].z - m1 - xh[it].z * m2), rs * (g[it].w - m1 - xh[it].w * m2));
                o.x += rr[it].x; o.y += rr[it].y; o.z += rr[it].z; o.w += rr[it].w;
                *reinterpret_cast<float4*>(dx32 + xr + c) = o;
                if (dx16) {
                    if (dmask.thresh) {          // residual dropout of the consumer c_proj: only its 16-bit operand copy is masked
                        const unsigned e = (unsigned)(xr + c);
                        float m0, m1, m2, m3;
                        drop_mul_pair(dmask, e, m0, m1);
                        drop_mul_pair(dmask, e + 2, m2, m3);
                        o.x *= m0; o.y *= m1; o.z *= m2; o.w *= m3;
                    }
                    const act_raw4 pk = act_pack4(o.x, o.y, o.z, o.w);
#if CC_OP == 2
                    if (img) {
                        uint2 hi, lo;
                        x3_pair4(o.x, o.y, o.z, o.w, hi, lo);
                        x3_store4(reinterpret_cast<op16_t*>(dx16) + 3 * (size_t)xr + c, D, hi, lo);
                    } else
#endif
                    act_straw4(dx16 + xr + c, pk);
                    if constexpr (DG) {
                        if (dcol) {
                            float r0, r1, r2, r3;
                            act_unpack4(pk, r0, r1, r2, r3);
                            pc[it].x += r0; pc[it].y += r1; pc[it].z += r2; pc[it].w += r3;
                        }
                    }
                }
            }
        }
        if constexpr (DG) { if (more) cur = nxt; } else { if (row + rstep < rows) fetch(row + rstep, cur); }
    }
    if constexpr (DG) {
        float* rg = ln_red;
        float* rb = ln_red + NW * D;
        float* pp = part + (size_t)blockIdx.x * (dcol ? 3 : 2) * D;      // this block's partials: [dgamma | dbeta | dcol]
#pragma unroll
        for (int it = 0; it < NV; it++) {
            const int c = ln_col(lane, it);
            if (c < D) {
                *reinterpret_cast<float4*>(rg + wave * D + c) = pg[it];
                *reinterpret_cast<float4*>(rb + wave * D + c) = pb[it];
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < D; c += NW * 64) {
            float sg = 0.f, sb = 0.f;
#pragma unroll
            for (int w = 0; w < NW; w++) { sg += rg[w * D + c]; sb += rb[w * D + c]; }
            pp[c] = sg;
            pp[D + c] = sb;
        }
        if (dcol) {                          // third reduction through the same buffer
            __syncthreads();
#pragma unroll
            for (int it = 0; it < NV; it++) {
                const int c = ln_col(lane, it);
                if (c < D) *reinterpret_cast<float4*>(rg + wave * D + c) = pc[it];
            }
            __syncthreads();
            for (int c = threadIdx.x; c < D; c += NW * 64) {
                float sc = 0.f;
#pragma unroll
                for (int w = 0; w < NW; w++) sc += rg[w * D + c];
                pp[2 * D + c] = sc;
            }
        }
    }
}
int ln_bwd(const act_t* dy, const float* x, int ldx, const int* row_map, const float* mean, const float* rstd,
           const float* gamma, const float* dres, float* dx32, Act dxo, float* dgamma, float* dbeta, int rows, int D,
           Call& cx, float* dcol, Drop dmask) {
    const hipStream_t st = cx.st;
    act_t* const dx16 = dxo.p;
    if (D > LN_MAXV * 256 || (D & 3) || (ldx & 3) || (dcol && (!dgamma || !dx16 || row_map)) || (dmask.thresh && (row_map || ldx != D)))
        return CC_ERR_SHAPE;
    if (rows <= 0) return CC_OK;
    // with parameter gradients every block ends with 2*D (3*D with dcol) partial sums that k_fold_partials folds in a fixed order: keep
    // the block count low (one per CU) so that the partials stay small, and give those blocks 8 waves
    const int nw = (dgamma && (size_t)16 * D * sizeof(float) <= 65536) ? 8 : 4;      // 8-wave reduction buffer within the 64 KiB default
    static const int dg_grid = []() { const char* e = cc_lab_env("CC_LNBWD_GRID"); return e ? atoi(e) : 256; }();   // tuning knob
    const int nvec = dcol ? 3 : 2;
    const int grid = std::min((rows + nw - 1) / nw, dgamma ? std::max(1, std::min(dg_grid, (int)(RED_SCRATCH_FLOATS / ((size_t)nvec * D)))) : 8192);
    float* part = dgamma ? red_scratch(cx, (size_t)grid * nvec * D) : nullptr;
    if (dgamma && !part) return CC_ERR_STATE;
    const size_t sh = dgamma ? (size_t)2 * nw * D * sizeof(float) : 0;
    const int img = dxo.img ? 1 : 0;          // the next GEMM reads dx16 as an operand image: either write one or fail loudly
    if (img && (!kX3 || dxo.img != D || ldx != D || dcol || dmask.thresh)) return CC_ERR_STATE;
#define LN_BWD(NV, DG, NW) hipLaunchKernelGGL((k_ln_bwd<NV, DG, NW>), dim3(grid), dim3(NW * 64), sh, st, dy, x, ldx, row_map, mean, rstd, gamma, dres, dx32, dx16, dgamma, dbeta, dcol, rows, D, dmask, img, part)
    if (dgamma && nw == 8) LN_NV(D, LN_BWD, true, 8) else if (dgamma) LN_NV(D, LN_BWD, true, 4) else LN_NV(D, LN_BWD, false, 4)
#undef LN_BWD
    if (!dgamma) return CC_OK;
    FoldOut o{};
    o.p[0] = dgamma; o.p[1] = dbeta; o.p[2] = dcol; o.m = D; o.k = nvec;
    return fold_partials(part, grid, nvec * D, 1, o, st);
}

}  // namespace CC_NS
