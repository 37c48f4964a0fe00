// HBM-/LDS-bound kernels of the ClipCap path for gfx950: conversions, LayerNorm fwd/bwd, deterministic reductions, dropout,
// embedding assembly, softmax-cross-entropy pieces, column sums, AdamW and the split-bf16 helpers.  Attention lives in attention.hip.
// All are wave64 code; memory accesses are 16-B vectors wherever the layout allows.
#include "kernels.h"
#include "gemm_api.h"

namespace CC_NS {

// ------------------------------------------------------------------------------------------------------------
// element-wise helpers
// ------------------------------------------------------------------------------------------------------------
__global__ void k_f32_to_bf16(const float* __restrict__ src, op16_t* __restrict__ dst, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const float4 a = reinterpret_cast<const float4*>(src)[2 * i], b = reinterpret_cast<const float4*>(src)[2 * i + 1];
        float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        reinterpret_cast<uint4*>(dst)[i] = pack8(v);
    }
}
int f32_to_bf16(const float* src, op16_t* dst, size_t n, hipStream_t st) {
    if (n & 7) return CC_ERR_SHAPE;
    const size_t n8 = n >> 3;
    if (!n8) return CC_OK;
    const int grid = (int)std::min<size_t>((n8 + 255) / 256, 2048);
    hipLaunchKernelGGL(k_f32_to_bf16, dim3(grid), dim3(256), 0, st, src, dst, n8);
    return CC_OK;
}

// gradient wire format of the N-rank all-reduce (train/ddp.py, bf16 wire): fp32 arena slice <-> bf16 staging slice, any length / alignment
// (a layer's slice starts wherever its first parameter does).  Always bf16 (round to nearest even), whatever the operand build.
__device__ __forceinline__ unsigned short wire_bf16(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);      // NaN stays NaN
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__global__ void k_wire_pack(const float* __restrict__ src, unsigned short* __restrict__ dst, size_t n) {
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * blockDim.x * 4) {
        if (i + 4 <= n && ((reinterpret_cast<size_t>(src + i) & 15) == 0) && ((reinterpret_cast<size_t>(dst + i) & 7) == 0)) {
            const float4 a = *reinterpret_cast<const float4*>(src + i);
            *reinterpret_cast<uint2*>(dst + i) = make_uint2(wire_bf16(a.x) | ((unsigned)wire_bf16(a.y) << 16), wire_bf16(a.z) | ((unsigned)wire_bf16(a.w) << 16));
        } else {
            for (size_t j = i; j < n && j < i + 4; j++) dst[j] = wire_bf16(src[j]);
        }
    }
}
__global__ void k_wire_unpack(const unsigned short* __restrict__ src, float* __restrict__ dst, size_t n) {
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * blockDim.x * 4) {
        if (i + 4 <= n && ((reinterpret_cast<size_t>(dst + i) & 15) == 0) && ((reinterpret_cast<size_t>(src + i) & 7) == 0)) {
            const uint2 a = *reinterpret_cast<const uint2*>(src + i);
            *reinterpret_cast<float4*>(dst + i) = make_float4(__uint_as_float(a.x << 16), __uint_as_float(a.x & 0xffff0000u), __uint_as_float(a.y << 16),
                                                              __uint_as_float(a.y & 0xffff0000u));
        } else {
            for (size_t j = i; j < n && j < i + 4; j++) dst[j] = __uint_as_float((unsigned)src[j] << 16);
        }
    }
}
int wire_pack(const float* src, unsigned short* dst, size_t n, hipStream_t st) {
    if (!n) return CC_OK;
    hipLaunchKernelGGL(k_wire_pack, dim3((int)std::min<size_t>((n / 4 + 255) / 256 + 1, 2048)), dim3(256), 0, st, src, dst, n);
    return CC_OK;
}
int wire_unpack(const unsigned short* src, float* dst, size_t n, hipStream_t st) {
    if (!n) return CC_OK;
    hipLaunchKernelGGL(k_wire_unpack, dim3((int)std::min<size_t>((n / 4 + 255) / 256 + 1, 2048)), dim3(256), 0, st, src, dst, n);
    return CC_OK;
}

int f32_to_act(const float* src, act_t* dst, size_t n, hipStream_t st) {
    if constexpr (kX3) {
        if (!n) return CC_OK;
        return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
    } else {
        return f32_to_bf16(src, reinterpret_cast<op16_t*>(dst), n, st);
    }
}

// dst[b*dst_stride + i] = (bf16) src[b*src_stride + i], i < len (len % 8 == 0)
__global__ void k_slice_f32_to_bf16(const float* __restrict__ src, size_t src_stride, act_t* __restrict__ dst,
                                    size_t dst_stride, int len8, int B) {
    const size_t total = (size_t)len8 * B;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / len8), c = (int)(i % len8);
        const float* s = src + b * src_stride + (size_t)c * 8;
        const float4 x = *reinterpret_cast<const float4*>(s), y = *reinterpret_cast<const float4*>(s + 4);
        float v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        act_st8(dst + b * dst_stride + (size_t)c * 8, v);
    }
}
int slice_f32_to_bf16(const float* src, size_t src_stride, act_t* dst, size_t dst_stride, int len, int B, hipStream_t st) {
    if (len & 7) return CC_ERR_SHAPE;
    const size_t total = (size_t)(len >> 3) * B;
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_slice_f32_to_bf16, dim3((int)std::min<size_t>((total + 255) / 256, 2048)), dim3(256), 0, st, src,
                       src_stride, dst, dst_stride, len >> 3, B);
    return CC_OK;
}

// dst[b*dst_stride + i] = src[i] (+ add[i])  — broadcast a learned block (prefix_const) into every sample
__global__ void k_broadcast_rows(float* __restrict__ dst, size_t dst_stride, const float* __restrict__ src, int len4, int B) {
    const size_t total = (size_t)len4 * B;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / len4), c = (int)(i % len4);
        reinterpret_cast<float4*>(dst + b * dst_stride)[c] = reinterpret_cast<const float4*>(src)[c];
    }
}
int broadcast_rows(float* dst, size_t dst_stride, const float* src, int len, int B, hipStream_t st) {
    if (len & 3) return CC_ERR_SHAPE;
    const size_t total = (size_t)(len >> 2) * B;
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_broadcast_rows, dim3((int)std::min<size_t>((total + 255) / 256, 2048)), dim3(256), 0, st, dst, dst_stride,
                       src, len >> 2, B);
    return CC_OK;
}

// dst[b*dst_stride + i] += add[i]  (positional embeddings of the windowed mapper)
__global__ void k_add_rows(float* __restrict__ dst, size_t dst_stride, const float* __restrict__ add, int len, int B) {
    const size_t total = (size_t)len * B;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / len), c = (int)(i % len);
        dst[b * dst_stride + c] += add[c];
    }
}
int add_rows(float* dst, size_t dst_stride, const float* add, int len, int B, hipStream_t st) {
    const size_t total = (size_t)len * B;
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_add_rows, dim3((int)std::min<size_t>((total + 255) / 256, 2048)), dim3(256), 0, st, dst, dst_stride, add, len, B);
    return CC_OK;
}

// ---- deterministic cross-block reductions (kernels.h): per-block partials in the call's scratch, folded in a fixed order ----
static float* red_scratch(const Call& cx, size_t floats) { return floats <= RED_SCRATCH_FLOATS ? cx.red : nullptr; }

// partials part[y][s][j] (y < gridDim.y groups of S slices x n columns): out[y * k + j / m][j % m] += sum over s of part[y][s][j], the
// slices summed in one fixed order: per chunk of 256 slices, lane g (of 16) of a column loads s = g, g + 16, ..., g + 240 at once and adds
// them as a fixed tree; the 16 lane sums are then added in lane order.
struct FoldOut { float* p[32]; int m; int k; };
__global__ __launch_bounds__(1024) void k_fold_partials(const float* __restrict__ part, int S, int n, FoldOut o) {
    __shared__ float red[16][64];
    const int t = threadIdx.x & 63, g = threadIdx.x >> 6, j = blockIdx.x * 64 + t;
    const float* __restrict__ src = part + (size_t)blockIdx.y * S * n;
    float acc = 0.f;
    if (j < n) {
        for (int k0 = 0; k0 < S; k0 += 256) {
            float v[16];
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int k = k0 + g + 16 * i;
                v[i] = k < S ? src[(size_t)k * n + j] : 0.f;
            }
#pragma unroll
            for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
                for (int i = 0; i < w; i++) v[i] += v[i + w];
            acc += v[0];
        }
    }
    red[g][t] = acc;
    __syncthreads();
    if (g == 0 && j < n) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 16; q++) s += red[q][t];
        o.p[blockIdx.y * o.k + j / o.m][j % o.m] += s;
    }
}
static int fold_partials(const float* part, int S, int n, int groups, const FoldOut& o, hipStream_t st) {
    hipLaunchKernelGGL(k_fold_partials, dim3((n + 63) / 64, groups), dim3(1024), 0, st, part, S, n, o);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

// dst[i] += sum_b src[b*src_stride + i]   (gradient of a broadcast block).  Grid = column blocks x batch slices: each thread sums its
// slice of the batch with 4 independent loads in flight; the slices' partial sums are folded in a fixed order by k_fold_partials (a
// single thread per column walking all B rows took 58 us for 256 x 7680 floats: 30 blocks, one load in flight each).
__global__ __launch_bounds__(256) void k_batch_sum(const float* __restrict__ src, size_t src_stride, float* __restrict__ dst, int len, int B,
                                                    int per, float* __restrict__ part) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const int b0 = blockIdx.y * per, b1 = min(B, b0 + per);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int b = b0;
    for (; b + 3 < b1; b += 4) {
        s0 += src[(size_t)b * src_stride + i];
        s1 += src[(size_t)(b + 1) * src_stride + i];
        s2 += src[(size_t)(b + 2) * src_stride + i];
        s3 += src[(size_t)(b + 3) * src_stride + i];
    }
    for (; b < b1; b++) s0 += src[(size_t)b * src_stride + i];
    const float s = (s0 + s1) + (s2 + s3);
    if (gridDim.y == 1) dst[i] += s;
    else part[(size_t)blockIdx.y * len + i] = s;
}
int batch_sum(const float* src, size_t src_stride, float* dst, int len, int B, Call& cx) {
    const hipStream_t st = cx.st;
    if (!len || B <= 0) return CC_OK;
    const int colb = (len + 255) / 256;
    int slices = std::max(1, std::min(B / 8, 1024 / colb));        // ~1k blocks, at least 8 rows per slice
    const int per = (B + slices - 1) / slices;
    slices = (B + per - 1) / per;
    float* part = slices > 1 ? red_scratch(cx, (size_t)slices * len) : nullptr;
    if (slices > 1 && !part) return CC_ERR_STATE;
    hipLaunchKernelGGL(k_batch_sum, dim3(colb, slices), dim3(256), 0, st, src, src_stride, dst, len, B, per, part);
    if (slices == 1) return CC_OK;
    FoldOut o{};
    o.p[0] = dst; o.m = len; o.k = 1;
    return fold_partials(part, slices, len, 1, o, st);
}

// dst[b*dst_stride + i] = src[b*src_stride + i]  fp32 strided copy (len % 4 == 0)
__global__ void k_copy_rows(const float* __restrict__ src, size_t src_stride, float* __restrict__ dst, size_t dst_stride, int len4, int B) {
    const size_t total = (size_t)len4 * B;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / len4), c = (int)(i % len4);
        reinterpret_cast<float4*>(dst + b * dst_stride)[c] = reinterpret_cast<const float4*>(src + b * src_stride)[c];
    }
}
int copy_rows(const float* src, size_t src_stride, float* dst, size_t dst_stride, int len, int B, hipStream_t st) {
    if (len & 3) return CC_ERR_SHAPE;
    const size_t total = (size_t)(len >> 2) * B;
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_copy_rows, dim3((int)std::min<size_t>((total + 255) / 256, 2048)), dim3(256), 0, st, src, src_stride, dst,
                       dst_stride, len >> 2, B);
    return CC_OK;
}

// dst[c][r] = src[r][c] for a bf16 matrix [R][C] (R, C multiples of 8): 64x64 tiles through LDS, 16-B global accesses both ways.
__global__ __launch_bounds__(256) void k_transpose_bf16(const op16_t* __restrict__ src, op16_t* __restrict__ dst, int R, int C) {
    __shared__ op16_t tile[64][66];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;  // 8 column groups x 32 rows, two passes
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int r = r0 + rl + 32 * p, c = c0 + cg * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r < R && c < C) v = *reinterpret_cast<const uint4*>(src + (size_t)r * C + c);
        const op16_t* e = reinterpret_cast<const op16_t*>(&v);
#pragma unroll
        for (int k = 0; k < 8; k++) tile[rl + 32 * p][cg * 8 + k] = e[k];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int c = c0 + rl + 32 * p, r = r0 + cg * 8;   // output row = source column
        if (c < C && r < R) {
            op16_t e[8];
#pragma unroll
            for (int k = 0; k < 8; k++) e[k] = tile[cg * 8 + k][rl + 32 * p];
            *reinterpret_cast<uint4*>(dst + (size_t)c * R + r) = *reinterpret_cast<const uint4*>(e);
        }
    }
}
// several matrices in one launch (the per-step weight sync transposes 4 small matrices per layer): blockIdx.z picks the matrix,
// blocks outside its extents exit
__global__ __launch_bounds__(256) void k_transpose_bf16_multi(TransposeBatch b) {
    const TransposeBatch::Item& m = b.it[blockIdx.z];
    if ((int)blockIdx.x * 64 >= m.C || (int)blockIdx.y * 64 >= m.R) return;
    __shared__ op16_t tile[64][66];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64, R = m.R, C = m.C;
    const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int r = r0 + rl + 32 * p, c = c0 + cg * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r < R && c < C) v = *reinterpret_cast<const uint4*>(m.src + (size_t)r * C + c);
        const op16_t* e = reinterpret_cast<const op16_t*>(&v);
#pragma unroll
        for (int k = 0; k < 8; k++) tile[rl + 32 * p][cg * 8 + k] = e[k];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int c = c0 + rl + 32 * p, r = r0 + cg * 8;
        if (c < C && r < R) {
            op16_t e[8];
#pragma unroll
            for (int k = 0; k < 8; k++) e[k] = tile[cg * 8 + k][rl + 32 * p];
            *reinterpret_cast<uint4*>(m.dst + (size_t)c * R + r) = *reinterpret_cast<const uint4*>(e);
        }
    }
}
int transpose_bf16_multi(const TransposeBatch& b, hipStream_t st) {
    if (b.n <= 0) return CC_OK;
    int mr = 0, mc = 0;
    for (int i = 0; i < b.n; i++) {
        if ((b.it[i].R & 7) || (b.it[i].C & 7)) return CC_ERR_SHAPE;
        mr = std::max(mr, b.it[i].R);
        mc = std::max(mc, b.it[i].C);
    }
    hipLaunchKernelGGL(k_transpose_bf16_multi, dim3((mc + 63) / 64, (mr + 63) / 64, b.n), dim3(256), 0, st, b);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}
int transpose_bf16(const op16_t* src, op16_t* dst, int R, int C, hipStream_t st) {
    if ((R & 7) || (C & 7)) return CC_ERR_SHAPE;
    if (R <= 0 || C <= 0) return CC_OK;
    hipLaunchKernelGGL(k_transpose_bf16, dim3((C + 63) / 64, (R + 63) / 64), dim3(256), 0, st, src, dst, R, C);
    return CC_OK;
}

// ------------------------------------------------------------------------------------------------------------
// LayerNorm forward: one wave per row, row cached in registers (D <= 2048, D % 4 == 0).
// y(bf16)[r] = (x[map(r)] - mean) * rstd * gamma + beta ; saves mean / rstd per output row.
// ------------------------------------------------------------------------------------------------------------
constexpr int LN_MAXV = 8;  // float4 per lane -> D <= 2048

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
            const int c = lane * 4 + it * 256;
            v[r][it] = c < D ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0, 0, 0, 0);
        }
    }
#pragma unroll
    for (int it = 0; it < NV; it++) {        // affine parameters fetched with the rows, not after the reductions
        const int c = lane * 4 + it * 256;
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
            const int c = lane * 4 + it * 256;
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
            const int c = lane * 4 + it * 256;
            if (c < D) {
                const float o0 = (v[r][it].x - mu[r]) * rs[r] * g[it].x + bt[it].x, o1 = (v[r][it].y - mu[r]) * rs[r] * g[it].y + bt[it].y;
                const float o2 = (v[r][it].z - mu[r]) * rs[r] * g[it].z + bt[it].z, o3 = (v[r][it].w - mu[r]) * rs[r] * g[it].w + bt[it].w;
#if CC_OP == 2
                if (y && img) {
                    const unsigned h01 = pack2op(o0, o1), h23 = pack2op(o2, o3);
                    float a0, a1, a2, a3;
                    unpack2(h01, a0, a1);
                    unpack2(h23, a2, a3);
                    const uint2 hi = make_uint2(h01, h23), lo = make_uint2(pack2op(o0 - a0, o1 - a1), pack2op(o2 - a2, o3 - a3));
                    op16_t* r3 = reinterpret_cast<op16_t*>(y) + (size_t)row * 3 * D + c;
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
    if (D <= 256) LN_FWD(1); else if (D <= 512) LN_FWD(2); else if (D <= 768) LN_FWD(3); else if (D <= 1024) LN_FWD(4); else LN_FWD(LN_MAXV);
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
        const int c = lane * 4 + it * 256;
        gmv[it] = c < D ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(0, 0, 0, 0);
    }
    struct RowIn { act_raw4 d[NV]; float4 xv[NV], rr[NV]; float mu, rs; size_t xr; };
    auto fetch = [&](int row, RowIn& r) {
        r.xr = (size_t)(row_map ? row_map[row] : row) * ldx;
        r.mu = mean[row]; r.rs = rstd[row];
#pragma unroll
        for (int it = 0; it < NV; it++) {
            const int c = lane * 4 + it * 256;
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
            const int c = lane * 4 + it * 256;
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
            const int c = lane * 4 + it * 256;
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
                        const unsigned h01 = pack2op(o.x, o.y), h23 = pack2op(o.z, o.w);
                        float a0, a1, a2, a3;
                        unpack2(h01, a0, a1);
                        unpack2(h23, a2, a3);
                        const uint2 hi = make_uint2(h01, h23), lo = make_uint2(pack2op(o.x - a0, o.y - a1), pack2op(o.z - a2, o.w - a3));
                        op16_t* r3 = reinterpret_cast<op16_t*>(dx16) + 3 * (size_t)xr + c;
                        *reinterpret_cast<uint2*>(r3) = hi;
                        *reinterpret_cast<uint2*>(r3 + D) = hi;
                        *reinterpret_cast<uint2*>(r3 + 2 * D) = lo;
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
            const int c = lane * 4 + it * 256;
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
                const int c = lane * 4 + it * 256;
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
#define LN_BWD_D(DG, NW) { if (D <= 256) LN_BWD(1, DG, NW); else if (D <= 512) LN_BWD(2, DG, NW); else if (D <= 768) LN_BWD(3, DG, NW); else if (D <= 1024) LN_BWD(4, DG, NW); else LN_BWD(LN_MAXV, DG, NW); }
    if (dgamma && nw == 8) LN_BWD_D(true, 8) else if (dgamma) LN_BWD_D(true, 4) else LN_BWD_D(false, 4)
#undef LN_BWD_D
#undef LN_BWD
    if (!dgamma) return CC_OK;
    FoldOut o{};
    o.p[0] = dgamma; o.p[1] = dbeta; o.p[2] = dcol; o.m = D; o.k = nvec;
    return fold_partials(part, grid, nvec * D, 1, o, st);
}

// ------------------------------------------------------------------------------------------------------------
// Column sums of a bf16 matrix (bias gradients): out[n] += sum_m X[m][n].  Block = 64 columns x a row slice.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_colsum_bf16(const act_t* __restrict__ X, int ld, int M, int N, float* __restrict__ out,
                                                     int rows_per_slice, float* __restrict__ part) {
    __shared__ float red[32][65];
    const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;
    const int col = blockIdx.x * 64 + cg * 8;
    const int r0 = blockIdx.y * rows_per_slice, r1 = min(M, r0 + rows_per_slice);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col < N) {
        for (int r = r0 + rl; r < r1; r += 32) {
            float f[8];
            act_ld8(X + (size_t)r * ld + col, f);
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] += f[e];
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
        if (c < N) {
            if (gridDim.y == 1) out[c] += s;
            else part[(size_t)blockIdx.y * N + c] = s;         // folded in a fixed order by k_fold_partials
        }
    }
}
// the same column sums for up to 32 equally shaped matrices in one launch (blockIdx.z = matrix): the mapper backward's per-layer
// fc1.bias gradients, deferred to the end of the call together with the weight gradients (round 5)
__global__ __launch_bounds__(256) void k_colsum_bf16_multi(ColsumBatch b, int ld, int M, int N, int rows_per_slice, float* __restrict__ part) {
    __shared__ float red[32][65];
    const act_t* __restrict__ X = b.X[blockIdx.z];
    float* __restrict__ out = b.out[blockIdx.z];
    const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;
    const int col = blockIdx.x * 64 + cg * 8;
    const int r0 = blockIdx.y * rows_per_slice, r1 = min(M, r0 + rows_per_slice);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col < N) {
        for (int r = r0 + rl; r < r1; r += 32) {
            float f[8];
            act_ld8(X + (size_t)r * ld + col, f);
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] += f[e];
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
        if (c < N) {
            if (gridDim.y == 1) out[c] += s;
            else part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * N + c] = s;
        }
    }
}
int colsum_bf16_multi(const ColsumBatch& b, int ld, int M, int N, Call& cx) {
    const hipStream_t st = cx.st;
    if ((N & 7) || (ld & 7) || b.n < 0 || b.n > 32) return CC_ERR_SHAPE;
    if (M <= 0 || N <= 0 || b.n == 0) return CC_OK;
    const int cb = (N + 63) / 64;
    int slices = std::max(1, std::min((M + 255) / 256, std::max(1, 1024 / (cb * b.n))));
    const int rps = ((M + slices - 1) / slices + 31) / 32 * 32;
    slices = (M + rps - 1) / rps;
    float* part = slices > 1 ? red_scratch(cx, (size_t)b.n * slices * N) : nullptr;
    if (slices > 1 && !part) return CC_ERR_STATE;
    hipLaunchKernelGGL(k_colsum_bf16_multi, dim3(cb, slices, b.n), dim3(256), 0, st, b, ld, M, N, rps, part);
    if (hipGetLastError() != hipSuccess) return CC_ERR_LAUNCH;
    if (slices == 1) return CC_OK;
    FoldOut o{};
    for (int i = 0; i < b.n; i++) o.p[i] = b.out[i];
    o.m = N; o.k = 1;
    return fold_partials(part, slices, N, b.n, o, st);
}
int colsum_bf16(const act_t* X, int ld, int M, int N, float* out, Call& cx) {
    const hipStream_t st = cx.st;
    if ((N & 7) || (ld & 7)) return CC_ERR_SHAPE;
    if (M <= 0 || N <= 0) return CC_OK;
    const int cb = (N + 63) / 64;
    int slices = std::max(1, std::min((M + 255) / 256, 1024 / cb));
    const int rps = ((M + slices - 1) / slices + 31) / 32 * 32;
    slices = (M + rps - 1) / rps;
    float* part = slices > 1 ? red_scratch(cx, (size_t)slices * N) : nullptr;
    if (slices > 1 && !part) return CC_ERR_STATE;
    hipLaunchKernelGGL(k_colsum_bf16, dim3(cb, slices), dim3(256), 0, st, X, ld, M, N, out, rps, part);
    if (slices == 1) return CC_OK;
    FoldOut o{};
    o.p[0] = out; o.m = N; o.k = 1;
    return fold_partials(part, slices, N, 1, o, st);
}

// ------------------------------------------------------------------------------------------------------------
// GPT-2 input assembly: x0[b,t,:] = (t < L ? prefix[b,t,:] : wte[tok[b,t-L],:]) + wpe[pos0 + t,:]   (fp32)
// (clipcap/model/model.py:45-49 + hf modeling_gpt2.py:571-577).  tokens < 0 (pads) are read as id 0 (model.py:104).
// ------------------------------------------------------------------------------------------------------------
// In-place dropout (common.hip.h: counter-based mask): embedding dropout on x0 / dx0 (fp32) and the masked bf16 copy of the residual
// gradient that feeds a c_proj backward.
// ------------------------------------------------------------------------------------------------------------
__global__ void k_dropout_f32(float* __restrict__ x, size_t n4, Drop d) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 v = reinterpret_cast<float4*>(x)[i];
        const unsigned e = (unsigned)(i * 4);
        float m0, m1, m2, m3;
        drop_mul_pair(d, e, m0, m1);
        drop_mul_pair(d, e + 2, m2, m3);
        v.x *= m0; v.y *= m1; v.z *= m2; v.w *= m3;
        reinterpret_cast<float4*>(x)[i] = v;
    }
}
__global__ void k_dropout_bf16(act_t* __restrict__ x, size_t n8, Drop d) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        float f[8];
        act_ld8(x + i * 8, f);
        const unsigned e = (unsigned)(i * 8);
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            float m0, m1;
            drop_mul_pair(d, e + k, m0, m1);
            f[k] *= m0; f[k + 1] *= m1;
        }
        act_st8(x + i * 8, f);
    }
}
__global__ void k_dropout_mask(unsigned char* __restrict__ out, size_t n, Drop d) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = (d.thresh == 0 || drop_keep(d, (unsigned)i)) ? 1 : 0;
}
int dropout_f32(float* x, size_t n, Drop d, hipStream_t st) {
    if (!d.thresh || !n) return CC_OK;
    if (n & 3) return CC_ERR_SHAPE;
    hipLaunchKernelGGL(k_dropout_f32, dim3((int)std::min<size_t>((n / 4 + 255) / 256, 4096)), dim3(256), 0, st, x, n / 4, d);
    return CC_OK;
}
int dropout_bf16(act_t* x, size_t n, Drop d, hipStream_t st) {
    if (!d.thresh || !n) return CC_OK;
    if (n & 7) return CC_ERR_SHAPE;
    hipLaunchKernelGGL(k_dropout_bf16, dim3((int)std::min<size_t>((n / 8 + 255) / 256, 4096)), dim3(256), 0, st, x, n / 8, d);
    return CC_OK;
}
int dropout_mask_u8(unsigned char* out, size_t n, Drop d, hipStream_t st) {
    if (!n) return CC_OK;
    hipLaunchKernelGGL(k_dropout_mask, dim3((int)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, out, n, d);
    return CC_OK;
}

// ------------------------------------------------------------------------------------------------------------
__global__ void k_embed_concat(const float* __restrict__ prefix, const long long* __restrict__ tokens, int cap,
                               const float* __restrict__ wte, const float* __restrict__ wpe, float* __restrict__ x0,
                               int B, int L, int T, int D, int pos0) {
    const int d4n = D >> 2;
    const size_t total = (size_t)B * T * d4n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % d4n);
        const int t = (int)((i / d4n) % T), b = (int)(i / ((size_t)d4n * T));
        float4 v;
        if (t < L)
            v = reinterpret_cast<const float4*>(prefix + ((size_t)b * L + t) * D)[c];
        else {
            long long id = tokens[(size_t)b * cap + (t - L)];
            if (id < 0) id = 0;
            v = reinterpret_cast<const float4*>(wte + (size_t)id * D)[c];
        }
        const float4 p = reinterpret_cast<const float4*>(wpe + (size_t)(pos0 + t) * D)[c];
        reinterpret_cast<float4*>(x0)[i] = make_float4(v.x + p.x, v.y + p.y, v.z + p.z, v.w + p.w);
    }
}
int embed_concat(const float* prefix, const long long* tokens, int cap, const float* wte, const float* wpe, float* x0, int B, int L,
                 int T, int D, int pos0, hipStream_t st) {
    if (D & 3) return CC_ERR_SHAPE;
    const size_t total = (size_t)B * T * (D >> 2);
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_embed_concat, dim3((int)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, st, prefix, tokens, cap,
                       wte, wpe, x0, B, L, T, D, pos0);
    return CC_OK;
}

// dst[r][c] = op16(src[r][c]) for c < V, 0 for V <= c < ldd (gradient of caller-visible fp32 logits -> the GEMM operand layout)
__global__ __launch_bounds__(256) void k_f32_to_op16_pad(const float* __restrict__ src, long long lds, int V, act_t* __restrict__ dst, int ldd,
                                                         int M) {
    const size_t total = (size_t)M * ldd;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % ldd);
        const size_t r = i / ldd;
        dst[i] = c < V ? f2act(src[r * lds + c]) : (act_t)0;
    }
}
int f32_to_op16_pad(const float* src, long long lds, int V, act_t* dst, int ldd, int M, hipStream_t st) {
    const size_t total = (size_t)M * ldd;
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_f32_to_op16_pad, dim3((int)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, st, src, lds, V, dst, ldd, M);
    return CC_OK;
}
// ---- deterministic token-indexed scatter-add (kernels.h scatter_rows, where the order is specified) ----
// Index: k_sc_sort_tile sorts the keys (id << 32 | row) of SC_TILE rows per workgroup in LDS (bitonic); k_sc_rank gives every key its place
// in the whole sorted array, the number of keys below it summed over the tiles (binary searches in LDS; the keys are unique), and the
// start and length of its id's list the same way; k_sc_compact (one workgroup) lists the chunk heads and the multi-chunk lists.  Sum:
// k_sc_sum, one wave per (chunk, 256 columns), each lane walking its 4 columns down the chunk in list order; k_sc_fold adds a multi-chunk
// list's partials in chunk order onto its row.  No atomics: every output element and every partial has exactly one writer.
namespace {
constexpr int SC_TILE = 2048;        // keys per LDS tile of the index sort
typedef unsigned long long sc_key;
struct ScatterWS {
    sc_key *tkeys, *skeys;
    int2* info;       // per sorted position: {start, length} of its id's list
    int *heads, *mstarts, *cnt;
    float* part;
    size_t bytes;
};
ScatterWS sc_carve(void* ws, int R, int D) {
    ScatterWS w{};
    char* base = static_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t n) { off = (off + 255) & ~size_t(255); char* r = base ? base + off : nullptr; off += n; return r; };
    w.tkeys = reinterpret_cast<sc_key*>(take((size_t)R * sizeof(sc_key)));
    w.skeys = reinterpret_cast<sc_key*>(take((size_t)R * sizeof(sc_key)));
    w.info = reinterpret_cast<int2*>(take((size_t)R * sizeof(int2)));
    w.heads = reinterpret_cast<int*>(take((size_t)R * sizeof(int)));
    w.mstarts = reinterpret_cast<int*>(take((size_t)(R / (SCATTER_CHUNK + 1) + 1) * sizeof(int)));
    w.cnt = reinterpret_cast<int*>(take(4 * sizeof(int)));
    // a list of n > CHUNK rows starting at sorted position s owns partial slots 2s/CHUNK + k, k < ceil(n/CHUNK): disjoint between lists
    // (floor(2(s+n)/C) >= floor(2s/C) + floor(2n/C) >= floor(2s/C) + ceil(n/C)) and below 2R/CHUNK
    w.part = reinterpret_cast<float*>(take((size_t)(2 * (size_t)R / SCATTER_CHUNK) * D * sizeof(float)));
    w.bytes = (off + 255) & ~size_t(255);
    return w;
}

template <bool ACT>
__device__ __forceinline__ void sc_row(const ScatterSrc& s, unsigned r, int D, int d0, float (&v)[4]) {
#pragma clang fp contract(off)
    if (ACT) {
        const float w = -s.fac[2 * (size_t)r + 1];
        const act_t* h = s.act + (size_t)r * D + d0;
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = w * act2f(h[e]);
    } else {
        const float* f = s.f32 + (size_t)(r / s.rpb) * s.bstride + (size_t)(r % s.rpb) * D + d0;
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = f[e];
    }
}

__global__ __launch_bounds__(1024) void k_sc_sort_tile(ScatterSrc s, int R, int Vp, int n, sc_key* __restrict__ tkeys) {
    __shared__ sc_key k[SC_TILE];
    const int base = blockIdx.x * SC_TILE;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int r = base + i;
        sc_key key = ~0ull;                                  // padding: above every real key, never stored
        if (r < R) {
            const size_t ir = (size_t)(r / s.rpb) * s.ids_ld + r % s.rpb;
            long long id = s.ids64 ? s.ids64[ir] : (long long)s.ids32[ir];
            id = id < 0 ? 0 : (id >= Vp ? Vp - 1 : id);
            unsigned hi = (unsigned)id;
            if (s.fac && s.fac[2 * (size_t)r + 1] == 0.f) hi = SC_SKIP;
            key = (sc_key)hi << 32 | (unsigned)r;
        }
        k[i] = key;
    }
    __syncthreads();
    for (int size = 2; size <= n; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += 1024) {
                const int p = i ^ j;
                if (p > i) {
                    const sc_key a = k[i], b = k[p];
                    if ((a > b) == ((i & size) == 0)) { k[i] = b; k[p] = a; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < n && base + i < R; i += 1024) tkeys[base + i] = k[i];
}

__global__ __launch_bounds__(256) void k_sc_rank(const sc_key* __restrict__ tkeys, int R, sc_key* __restrict__ skeys, int2* __restrict__ info) {
    __shared__ sc_key t[SC_TILE];
    const int p = blockIdx.x * 256 + threadIdx.x;
    const sc_key key = p < R ? tkeys[p] : ~0ull;
    const unsigned hi = (unsigned)(key >> 32);
    const sc_key lo_key = (sc_key)hi << 32, hi_key = hi == SC_SKIP ? ~0ull : (sc_key)(hi + 1) << 32;
    int pos = 0, ls = 0, le = 0;
    for (int base = 0; base < R; base += SC_TILE) {
        const int n = min(SC_TILE, R - base);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) t[i] = tkeys[base + i];
        __syncthreads();
        int a = 0, b = 0, c = 0;                             // counts of tile keys below key / lo_key / hi_key, three searches in step
        for (int step = SC_TILE; step > 0; step >>= 1) {
            if (a + step <= n && t[a + step - 1] < key) a += step;
            if (b + step <= n && t[b + step - 1] < lo_key) b += step;
            if (c + step <= n && t[c + step - 1] < hi_key) c += step;
        }
        pos += a; ls += b; le += c;
    }
    if (p >= R) return;
    skeys[pos] = key;
    info[pos] = make_int2(ls, hi == SC_SKIP ? 0 : le - ls);
}

// one workgroup: thread i takes sorted positions [i*span, (i+1)*span); counts, an exclusive scan of the counts, then the lists in order
__global__ __launch_bounds__(1024) void k_sc_compact(const sc_key* __restrict__ skeys, const int2* __restrict__ info, int R, int* __restrict__ heads,
                                                     int* __restrict__ mstarts, int* __restrict__ cnt) {
    __shared__ int sh[1024], sm[1024];
    const int tid = threadIdx.x, span = (R + 1023) / 1024, a = min(R, tid * span), b = min(R, a + span);
    int nh = 0, nm = 0;
    for (int p = a; p < b; p++) {
        const int2 li = info[p];
        const int off = p - li.x;
        if ((unsigned)(skeys[p] >> 32) == SC_SKIP || off % SCATTER_CHUNK) continue;
        nh++;
        nm += off == 0 && li.y > SCATTER_CHUNK;
    }
    sh[tid] = nh; sm[tid] = nm;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int x = tid >= d ? sh[tid - d] : 0, y = tid >= d ? sm[tid - d] : 0;
        __syncthreads();
        sh[tid] += x; sm[tid] += y;
        __syncthreads();
    }
    int oh = sh[tid] - nh, om = sm[tid] - nm;
    if (tid == 1023) { cnt[0] = sh[tid]; cnt[1] = sm[tid]; }
    for (int p = a; p < b; p++) {
        const int2 li = info[p];
        const int off = p - li.x;
        if ((unsigned)(skeys[p] >> 32) == SC_SKIP || off % SCATTER_CHUNK) continue;
        heads[oh++] = p;
        if (off == 0 && li.y > SCATTER_CHUNK) mstarts[om++] = p;
    }
}

template <bool ACT>
__global__ __launch_bounds__(256) void k_sc_sum(ScatterSrc s, const sc_key* __restrict__ skeys, const int2* __restrict__ info,
                                                const int* __restrict__ heads, const int* __restrict__ cnt, int D, int ncb,
                                                float* __restrict__ dst, float* __restrict__ part) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int items = cnt[0] * ncb;
    for (int it = blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += gridDim.x * 4) {
        const int h = it / ncb, d0 = (it % ncb) * 256 + lane * 4;
        const int p = heads[h];
        const int2 li = info[p];
        const int end = min(p + SCATTER_CHUNK, li.x + li.y);
        if (d0 >= D) continue;
        float acc[4];
        sc_row<ACT>(s, (unsigned)skeys[p], D, d0, acc);
        int q = p + 1;
        for (; q + 3 < end; q += 4) {                       // four rows' loads in flight, added in list order
            float v0[4], v1[4], v2[4], v3[4];
            sc_row<ACT>(s, (unsigned)skeys[q], D, d0, v0);
            sc_row<ACT>(s, (unsigned)skeys[q + 1], D, d0, v1);
            sc_row<ACT>(s, (unsigned)skeys[q + 2], D, d0, v2);
            sc_row<ACT>(s, (unsigned)skeys[q + 3], D, d0, v3);
#pragma unroll
            for (int e = 0; e < 4; e++) acc[e] = (((acc[e] + v0[e]) + v1[e]) + v2[e]) + v3[e];
        }
        for (; q < end; q++) {
            float v[4];
            sc_row<ACT>(s, (unsigned)skeys[q], D, d0, v);
#pragma unroll
            for (int e = 0; e < 4; e++) acc[e] += v[e];
        }
        float* o;
        if (li.y <= SCATTER_CHUNK) o = dst + (size_t)(skeys[p] >> 32) * D + d0;
        else o = part + (size_t)(2 * (size_t)li.x / SCATTER_CHUNK + (p - li.x) / SCATTER_CHUNK) * D + d0;
        if (li.y <= SCATTER_CHUNK) {
#pragma unroll
            for (int e = 0; e < 4; e++) o[e] = o[e] + acc[e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) o[e] = acc[e];
        }
    }
}

__global__ __launch_bounds__(256) void k_sc_fold(const sc_key* __restrict__ skeys, const int2* __restrict__ info, const int* __restrict__ mstarts,
                                                 const int* __restrict__ cnt, int D, int ncb, const float* __restrict__ part, float* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int items = cnt[1] * ncb;
    for (int it = blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += gridDim.x * 4) {
        const int m = it / ncb, d0 = (it % ncb) * 256 + lane * 4;
        if (d0 >= D) continue;
        const int p = mstarts[m];
        const int n = info[p].y, nk = (n + SCATTER_CHUNK - 1) / SCATTER_CHUNK;
        const float* src = part + (size_t)(2 * (size_t)p / SCATTER_CHUNK) * D + d0;
        float t[4];
#pragma unroll
        for (int e = 0; e < 4; e++) t[e] = src[e];
        for (int k = 1; k < nk; k++)
#pragma unroll
            for (int e = 0; e < 4; e++) t[e] += src[(size_t)k * D + e];
        float* o = dst + (size_t)(skeys[p] >> 32) * D + d0;
#pragma unroll
        for (int e = 0; e < 4; e++) o[e] = o[e] + t[e];
    }
}
}  // namespace

size_t scatter_ws_bytes(int R, int D) { return R > 0 ? sc_carve(nullptr, R, D).bytes : 0; }

int scatter_rows(const ScatterSrc& s, int R, int D, int Vp, float* dst, void* ws, hipStream_t st) {
    if (R < 0 || D <= 0 || (D & 3) || Vp <= 0 || (!s.ids32 && !s.ids64) || (!s.f32 && !(s.act && s.fac)) || s.rpb <= 0) return CC_ERR_ARG;
    if (R == 0) return CC_OK;
    if (!ws) return CC_ERR_STATE;
    const ScatterWS w = sc_carve(ws, R, D);
    const int nt = (R + SC_TILE - 1) / SC_TILE;
    int n = SC_TILE;
    if (nt == 1) for (n = 1; n < R; n <<= 1) {}
    hipLaunchKernelGGL(k_sc_sort_tile, dim3(nt), dim3(1024), 0, st, s, R, Vp, n, w.tkeys);
    hipLaunchKernelGGL(k_sc_rank, dim3((R + 255) / 256), dim3(256), 0, st, w.tkeys, R, w.skeys, w.info);
    hipLaunchKernelGGL(k_sc_compact, dim3(1), dim3(1024), 0, st, w.skeys, w.info, R, w.heads, w.mstarts, w.cnt);
    const int ncb = (D + 255) / 256;
    const int sum_blocks = (int)std::min<size_t>(((size_t)R * ncb + 3) / 4, 4096);
    if (s.act) hipLaunchKernelGGL(k_sc_sum<true>, dim3(sum_blocks), dim3(256), 0, st, s, w.skeys, w.info, w.heads, w.cnt, D, ncb, dst, w.part);
    else hipLaunchKernelGGL(k_sc_sum<false>, dim3(sum_blocks), dim3(256), 0, st, s, w.skeys, w.info, w.heads, w.cnt, D, ncb, dst, w.part);
    if (R > SCATTER_CHUNK) {
        const int fold_blocks = (int)std::min<size_t>(((size_t)(R / (SCATTER_CHUNK + 1) + 1) * ncb + 3) / 4, 1024);
        hipLaunchKernelGGL(k_sc_fold, dim3(fold_blocks), dim3(256), 0, st, w.skeys, w.info, w.mstarts, w.cnt, D, ncb, w.part, dst);
    }
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

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
__global__ __launch_bounds__(256) void k_ce_rows(const float* __restrict__ pmax, const float* __restrict__ psum, int npart,
                                                 const int* __restrict__ target, const float* __restrict__ tgt_logit,
                                                 float* __restrict__ lse, float* __restrict__ row_loss, int M) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float m, s;
    ce_row_fold(pmax, psum, npart, row, lane, m, s);
    if (lane == 0) {
        const float l = m + logf(s);
        lse[row] = l;
        row_loss[row] = (target[row] != 0) ? l - tgt_logit[row] : 0.f;
    }
}
// stats[0] = sum of kept-row losses, stats[1] = kept rows — one block, fixed summation order (deterministic, no atomics)
__global__ __launch_bounds__(1024) void k_ce_stats(const float* __restrict__ row_loss, const int* __restrict__ target, float* __restrict__ stats,
                                                   int M) {
    __shared__ float sl[16], sc[16];
    float a = 0.f, c = 0.f;
    for (int i = threadIdx.x; i < M; i += 1024) {
        a += row_loss[i];
        c += (target[i] != 0) ? 1.f : 0.f;
    }
    a = wave_sum(a);
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) { sl[threadIdx.x >> 6] = a; sc[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float ta = 0.f, tc = 0.f;
        for (int w = 0; w < 16; w++) { ta += sl[w]; tc += sc[w]; }
        stats[0] = ta;
        stats[1] = tc;
    }
}
int ce_rows(const float* pmax, const float* psum, int npart, const int* target, const float* tgt_logit, float* lse, float* row_loss,
            float* stats, int M, hipStream_t st) {
    if (M <= 0) return CC_OK;
    hipLaunchKernelGGL(k_ce_rows, dim3((M + 3) / 4), dim3(256), 0, st, pmax, psum, npart, target, tgt_logit, lse, row_loss, M);
    hipLaunchKernelGGL(k_ce_stats, dim3(1), dim3(1024), 0, st, row_loss, target, stats, M);
    return CC_OK;
}

// Scoring (cc_lmhead_score): token_logprob[row] = tgt_logit - lse for kept rows, 0 for the others; lse from the same fold as k_ce_rows.
__global__ __launch_bounds__(256) void k_score_rows(const float* __restrict__ pmax, const float* __restrict__ psum, int npart,
                                                    const int* __restrict__ keep, const float* __restrict__ tgt_logit,
                                                    float* __restrict__ lse, float* __restrict__ token_logprob, int M) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float m, s;
    ce_row_fold(pmax, psum, npart, row, lane, m, s);
    if (lane == 0) {
        const float l = m + logf(s);
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
__global__ __launch_bounds__(256) void k_ce_dlogits(act_t* __restrict__ logits, int ld, int V, const int* __restrict__ target,
                                                    const float* __restrict__ lse, const float* __restrict__ denom,
                                                    const float* __restrict__ loss_scale, int M, op16_t* __restrict__ img) {
    const int col = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (col >= ld) return;
    const float inv = (loss_scale ? loss_scale[0] : 1.0f) / fmaxf(denom[0], 1.0f);
    for (int row = blockIdx.y; row < M; row += gridDim.y) {
        const int t = target[row];
        const float l = lse[row];
        const float w = (t != 0) ? inv : 0.f;
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
            const uint4 hi = pack8(f);
            float h[8], d[8];
            unpack8(hi, h);
#pragma unroll
            for (int e = 0; e < 8; e++) d[e] = f[e] - h[e];
            const uint4 lo = pack8(d);
            op16_t* r3 = img + (size_t)row * 3 * ld + col;
            *reinterpret_cast<uint4*>(r3) = hi;
            *reinterpret_cast<uint4*>(r3 + ld) = hi;
            *reinterpret_cast<uint4*>(r3 + 2 * ld) = lo;
            continue;
        }
#endif
        act_st8(p, f);
    }
}
int ce_dlogits(act_t* logits, int ld, int V, const int* target, const float* lse, const float* denom, const float* loss_scale, int M,
               hipStream_t st, op16_t* img) {
    if (ld & 7) return CC_ERR_SHAPE;
    if (M <= 0) return CC_OK;
    hipLaunchKernelGGL(k_ce_dlogits, dim3((ld / 8 + 255) / 256, std::min(M, 32768)), dim3(256), 0, st, logits, ld, V, target, lse, denom, loss_scale, M, img);
    return CC_OK;
}

// ---- exponential form of the lm_head outputs (gemm.hip.h EpiLMHead): row helpers, one wave per row ----
__global__ __launch_bounds__(256) void k_lm_tgt_ref(const act_t* __restrict__ hf, const op16_t* __restrict__ wte, int D, const int* __restrict__ target,
                                                    float* __restrict__ cref, int M) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const act_t* h = hf + (size_t)row * D;
#if CC_OP == 2
    const float* w = reinterpret_cast<const float*>(wte) + (size_t)target[row] * D;     // bf16x3: the fp32 master row (what hi + lo stand for)
#else
    const op16_t* w = wte + (size_t)target[row] * D;
#endif
    float acc = 0.f;
    for (int d = lane * 8; d < D; d += 512) {
        float a[8], b[8];
        act_ld8(h + d, a);
#if CC_OP == 2
        act_ld8(w + d, b);
#else
        unpack8(*reinterpret_cast<const uint4*>(w + d), b);
#endif
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
__global__ void k_lm_rowfac(const float* __restrict__ cref, const float* __restrict__ lse, const int* __restrict__ target,
                            const float* __restrict__ denom, const float* __restrict__ loss_scale, float* __restrict__ fac, int M) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float inv = (loss_scale ? loss_scale[0] : 1.0f) / fmaxf(denom[0], 1.0f);
    const float w = target[i] != 0 ? inv : 0.f;
    fac[2 * i] = w != 0.f ? __expf(cref[i] - lse[i]) * w : 0.f;
    fac[2 * i + 1] = w;
}
int lm_rowfac(const float* cref, const float* lse, const int* target, const float* denom, const float* loss_scale, float* fac, int M, hipStream_t st) {
    if (M <= 0) return CC_OK;
    hipLaunchKernelGGL(k_lm_rowfac, dim3((M + 255) / 256), dim3(256), 0, st, cref, lse, target, denom, loss_scale, fac, M);
    return CC_OK;
}
// MODE 0: dhf = r dhf - w wte[t];  1: out = r hf
template <int MODE>
__global__ __launch_bounds__(256) void k_lm_rows(act_t* __restrict__ io, const act_t* __restrict__ hf, const float* __restrict__ fac,
                                                 const int* __restrict__ target, const op16_t* __restrict__ wte, float* __restrict__ dwte, int D, int M) {
    const int d8n = D >> 3;
    const size_t total = (size_t)M * d8n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / d8n), c = (int)(i % d8n) * 8;
        const float r = fac[2 * row], w = fac[2 * row + 1];
        float v[8];
        if (MODE == 0) {
            float b[8];
            act_ld8(io + (size_t)row * D + c, v);
#if CC_OP == 2
            act_ld8(reinterpret_cast<const float*>(wte) + (size_t)target[row] * D + c, b);
#else
            unpack8(*reinterpret_cast<const uint4*>(wte + (size_t)target[row] * D + c), b);
#endif
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = r * v[e] - w * b[e];
            act_st8(io + (size_t)row * D + c, v);
        } else {
            act_ld8(hf + (size_t)row * D + c, v);
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] *= r;
            act_st8(io + (size_t)row * D + c, v);
        }
    }
}
template <int MODE>
static int lm_rows_launch(act_t* io, const act_t* hf, const float* fac, const int* target, const op16_t* wte, float* dwte, int D, int M, hipStream_t st) {
    if (D & 7) return CC_ERR_SHAPE;
    const size_t total = (size_t)M * (D >> 3);
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_lm_rows<MODE>, dim3((int)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, st, io, hf, fac, target, wte, dwte, D, M);
    return CC_OK;
}
int lm_dgrad_fix(act_t* dhf, const float* fac, const int* target, const op16_t* wte, int D, int M, hipStream_t st) {
    return lm_rows_launch<0>(dhf, nullptr, fac, target, wte, nullptr, D, M, st);
}
int lm_scale_rows(const act_t* hf, const float* fac, act_t* out, int D, int M, hipStream_t st) {
    return lm_rows_launch<1>(out, hf, fac, nullptr, nullptr, nullptr, D, M, st);
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

// ------------------------------------------------------------------------------------------------------------
// Flat AdamW (torch.optim.AdamW math, decoupled decay) over one parameter arena.  HBM-bound: 16 B read + 12 B written per
// parameter.  inv_scale (device, nullable) = loss scale to divide out of the gradients; found_inf (device, nullable) != 0 skips
// the whole step (the GradScaler rule for an overflowed fp16 backward).
// ------------------------------------------------------------------------------------------------------------
template <bool DEVSTEP>      // DEVSTEP: Adam's step number is read from the loss scaler's device-side count (a separate instantiation: the
                             // pow evaluation must not cost the common kernel its registers — it measured 184 -> 223 us as a run-time branch)
__global__ __launch_bounds__(256) void k_adamw(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, size_t n4, float lr, float b1, float b2, float eps, float wd, float bc1,
                                               float bc2_sqrt, float gscale, const float* __restrict__ loss_scale,
                                               const float* __restrict__ found_inf, op16_t* __restrict__ w16,
                                               const float* __restrict__ clip) {
    if (found_inf && found_inf[0] != 0.f) return;
    if (loss_scale) gscale /= loss_scale[0];
    if (clip) gscale *= clip[0];      // global-norm clip coefficient (k_grad_clip_coef); 1.0f leaves gscale's bits as they are
    if constexpr (DEVSTEP) {      // step number = 1 + the loss scaler's count of APPLIED steps (loss_scale[2]): a skipped step does not advance Adam's bias correction
        const float t = loss_scale[2] + 1.0f;
        bc1 = 1.0f - __builtin_amdgcn_exp2f(t * __log2f(b1));
        bc2_sqrt = sqrtf(1.0f - __builtin_amdgcn_exp2f(t * __log2f(b2)));
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 P = reinterpret_cast<float4*>(p)[i], G = reinterpret_cast<const float4*>(g)[i];
        float4 M = reinterpret_cast<float4*>(m)[i], V = reinterpret_cast<float4*>(v)[i];
        float* pp = &P.x; float* gg = &G.x; float* mm = &M.x; float* vv = &V.x;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float gr = gg[e] * gscale;
            pp[e] *= (1.0f - lr * wd);
            mm[e] = b1 * mm[e] + (1.0f - b1) * gr;
            vv[e] = b2 * vv[e] + (1.0f - b2) * gr * gr;
            const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
            pp[e] -= (lr / bc1) * (mm[e] / denom);
        }
        reinterpret_cast<float4*>(p)[i] = P;
        reinterpret_cast<float4*>(m)[i] = M;
        reinterpret_cast<float4*>(v)[i] = V;
        // the 16-bit operand copy of the updated parameters, while they are in registers: saves the separate cast pass over the arena
        if (w16) reinterpret_cast<uint2*>(w16)[i] = make_uint2(pack2op(P.x, P.y), pack2op(P.z, P.w));
    }
}
int adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps, float wd, int step, float gscale,
          const float* loss_scale, const float* found_inf, hipStream_t st, op16_t* w16, const float* clip) {
    if (n & 3) return CC_ERR_SHAPE;
    if (!n) return CC_OK;
    if (step < 1 && !loss_scale) return CC_ERR_ARG;
    const float bc1 = 1.0f - powf(b1, (float)std::max(step, 1));
    const float bc2s = sqrtf(1.0f - powf(b2, (float)std::max(step, 1)));
    const size_t n4 = n >> 2;
    const dim3 gr((int)std::min<size_t>((n4 + 255) / 256, 4096));
    if (step < 1) hipLaunchKernelGGL(k_adamw<true>, gr, dim3(256), 0, st, p, g, m, v, n4, lr, b1, b2, eps, wd, bc1, bc2s, gscale, loss_scale, found_inf, w16, clip);
    else hipLaunchKernelGGL(k_adamw<false>, gr, dim3(256), 0, st, p, g, m, v, n4, lr, b1, b2, eps, wd, bc1, bc2s, gscale, loss_scale, found_inf, w16, clip);
    return CC_OK;
}

// ---- dynamic loss scaling (fp16 operands; torch.cuda.amp.GradScaler semantics, all on the device) ----
__global__ __launch_bounds__(256) void k_grad_nonfinite(const float* __restrict__ g, size_t n4, float* __restrict__ found_inf) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 G = reinterpret_cast<const float4*>(g)[i];
        // (x - x) is 0 for finite x and NaN for inf / NaN
        const float z = (G.x - G.x) + (G.y - G.y) + (G.z - G.z) + (G.w - G.w);
        bad |= !(z == 0.f);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) found_inf[0] = 1.0f;      // benign race: every writer stores the same value
}
int grad_nonfinite(const float* g, size_t n, float* found_inf, hipStream_t st) {
    if (n & 3) return CC_ERR_SHAPE;
    if (!n) return CC_OK;
    const size_t n4 = n >> 2;
    hipLaunchKernelGGL(k_grad_nonfinite, dim3((int)std::min<size_t>((n4 + 255) / 256, 2048)), dim3(256), 0, st, g, n4, found_inf);
    return CC_OK;
}
__global__ void k_loss_scale_update(float* state, float* found_inf, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (found_inf[0] != 0.f) {
        state[0] = fmaxf(state[0] * backoff, 1.0f);
        state[1] = 0.f;
    } else {
        const float good = state[1] + 1.f;
        if (good >= (float)interval) {
            state[0] = fminf(state[0] * growth, 16777216.0f);
            state[1] = 0.f;
        } else {
            state[1] = good;
        }
        state[2] += 1.f;      // optimizer steps actually applied (read by the next cc_adamw_step called with step = 0)
    }
    found_inf[0] = 0.f;
}
int loss_scale_update(float* state, float* found_inf, float growth, float backoff, int interval, hipStream_t st) {
    hipLaunchKernelGGL(k_loss_scale_update, dim3(1), dim3(64), 0, st, state, found_inf, growth, backoff, interval);
    return CC_OK;
}

// ---- global gradient norm + clip coefficient (torch.nn.utils.clip_grad_norm_, all on the device) ----
// sumsq[0] += sum g[i]^2 over a flat fp32 slice.  HBM-bound: 4 B read per parameter (AdamW moves 28).  Streaming-reduction shape: 16-byte
// loads, GRAD_NORM_ACC independent accumulators per thread (that many loads in flight), DPP wave_sum, cross-wave fold through LDS, one
// partial per block; a second, single-block launch folds the partials.  No atomics: the order is fixed by n alone (kernels.h states it).
__device__ __forceinline__ float sq4(const float4 G) { return (G.x * G.x + G.y * G.y) + (G.z * G.z + G.w * G.w); }
__global__ __launch_bounds__(GRAD_NORM_THREADS) void k_grad_sqnorm(const float* __restrict__ g, size_t n4, float* __restrict__ part) {
    static_assert(GRAD_NORM_THREADS == 256 && GRAD_NORM_ACC == 4, "the fold below is written for 4 waves and 4 accumulators");
    __shared__ float red[4];
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const size_t S = (size_t)gridDim.x * GRAD_NORM_THREADS;
    size_t i = (size_t)blockIdx.x * GRAD_NORM_THREADS + threadIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (; i + 3 * S < n4; i += 4 * S) {      // four visits per round: the loads are independent, each feeds its own accumulator
        const float4 G0 = g4[i], G1 = g4[i + S], G2 = g4[i + 2 * S], G3 = g4[i + 3 * S];
        a0 += sq4(G0); a1 += sq4(G1); a2 += sq4(G2); a3 += sq4(G3);
    }
    if (i < n4) a0 += sq4(g4[i]);             // the last (partial) round: visit k still goes to accumulator k % 4
    if (i + S < n4) a1 += sq4(g4[i + S]);
    if (i + 2 * S < n4) a2 += sq4(g4[i + 2 * S]);
    // every lane reaches the reduction (no early exit; a lane without elements brings 0): wave_sum's full-wave precondition
    const float w = wave_sum((a0 + a1) + (a2 + a3));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(GRAD_NORM_THREADS) void k_grad_sqnorm_fold(const float* __restrict__ part, int nb, float* __restrict__ sumsq) {
    __shared__ float red[4];
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < GRAD_NORM_BLOCKS / GRAD_NORM_THREADS; e++) {      // thread t: its run of consecutive partials, in index order
        const int j = threadIdx.x * (GRAD_NORM_BLOCKS / GRAD_NORM_THREADS) + e;
        if (j < nb) s += part[j];
    }
    const float w = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) sumsq[0] += (red[0] + red[1]) + (red[2] + red[3]);
}
int grad_sqnorm(const float* g, size_t n, float* scratch, float* sumsq, hipStream_t st) {
    if (n & 3) return CC_ERR_SHAPE;
    if (!n) return CC_OK;
    const size_t n4 = n >> 2;
    const int nb = (int)std::min<size_t>((n4 + GRAD_NORM_THREADS - 1) / GRAD_NORM_THREADS, GRAD_NORM_BLOCKS);
    hipLaunchKernelGGL(k_grad_sqnorm, dim3(nb), dim3(GRAD_NORM_THREADS), 0, st, g, n4, scratch);
    hipLaunchKernelGGL(k_grad_sqnorm_fold, dim3(1), dim3(GRAD_NORM_THREADS), 0, st, scratch, nb, sumsq);
    return CC_OK;
}
// clip[1] = the true (unscaled) norm, clip[0] = min(1, max_norm / (norm + 1e-6)); a non-finite norm gives a NaN coefficient
__global__ void k_grad_clip_coef(const float* sumsq, float max_norm, float grad_scale, const float* loss_scale, float* clip) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float norm = sqrtf(sumsq[0]) * grad_scale;
    if (loss_scale) norm /= loss_scale[0];
    clip[1] = norm;
    clip[0] = (norm - norm == 0.f) ? fminf(1.0f, max_norm / (norm + 1e-6f)) : __builtin_nanf("");
}
int grad_clip_coef(const float* sumsq, float max_norm, float grad_scale, const float* loss_scale, float* clip, hipStream_t st) {
    hipLaunchKernelGGL(k_grad_clip_coef, dim3(1), dim3(64), 0, st, sumsq, max_norm, grad_scale, loss_scale, clip);
    return CC_OK;
}

#if CC_OP == 2
// ------------------------------------------------------------------------------------------------------------
// bf16x3 operand pairs (common.hip.h): x -> hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32), laid out along K so that the
// unchanged NT kernels, run over K' = 3K, compute hi*hi + hi*lo + lo*hi:  A operand [hi | hi | lo],  B operand [hi | lo | hi].
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void x3_pair8(const float (&f)[8], uint4& hi, uint4& lo) {
    hi = pack8(f);
    float h[8], d[8];
    unpack8(hi, h);
#pragma unroll
    for (int e = 0; e < 8; e++) d[e] = f[e] - h[e];
    lo = pack8(d);
}
__device__ __forceinline__ void x3_store(op16_t* row3, int K, int c, int form, const uint4& hi, const uint4& lo) {
    *reinterpret_cast<uint4*>(row3 + c) = hi;
    *reinterpret_cast<uint4*>(row3 + K + c) = form ? lo : hi;
    *reinterpret_cast<uint4*>(row3 + 2 * K + c) = form ? hi : lo;
}
__global__ __launch_bounds__(256) void k_x3_split_rows(const float* __restrict__ src, size_t lds, op16_t* __restrict__ dst, int M, int K, int form) {
    const int k8 = K >> 3;
    const size_t total = (size_t)M * k8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / k8;
        const int c = (int)(i - r * k8) * 8;
        const float* sp = src + r * lds + c;
        const float4 a = *reinterpret_cast<const float4*>(sp), b = *reinterpret_cast<const float4*>(sp + 4);
        const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint4 hi, lo;
        x3_pair8(f, hi, lo);
        x3_store(dst + r * 3 * (size_t)K, K, c, form, hi, lo);
    }
}
int x3_split_rows(const float* src, size_t lds, op16_t* dst, int M, int K, int form, hipStream_t st) {
    if ((K & 7) || (lds & 3) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return CC_ERR_SHAPE;
    const size_t total = (size_t)M * (K >> 3);
    if (!total) return CC_OK;
    hipLaunchKernelGGL(k_x3_split_rows, dim3((int)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, st, src, lds, dst, M, K, form);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}
// weights: 64 x 64 source tiles; tr = 1 goes through LDS so that both the fp32 reads and the 16-bit writes are row-contiguous
__global__ __launch_bounds__(256) void k_x3_split_multi(X3SplitBatch b) {
    const X3SplitBatch::Item& m = b.it[blockIdx.z];
    if ((int)blockIdx.x * 64 >= m.C || (int)blockIdx.y * 64 >= m.R) return;
    __shared__ float tile[64][65];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64, R = m.R, C = m.C;
    const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;      // 8 chunks of 8 columns x 32 rows, two passes
    if (!m.tr) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const int r = r0 + rl + 32 * p, c = c0 + cg * 8;
            if (r < R && c < C) {
                const float* sp = m.src + (size_t)r * C + c;
                const float4 a = *reinterpret_cast<const float4*>(sp), bb = *reinterpret_cast<const float4*>(sp + 4);
                const float f[8] = {a.x, a.y, a.z, a.w, bb.x, bb.y, bb.z, bb.w};
                uint4 hi, lo;
                x3_pair8(f, hi, lo);
                x3_store(m.dst + (size_t)r * 3 * C, C, c, m.form, hi, lo);
            }
        }
        return;
    }
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int r = r0 + rl + 32 * p, c = c0 + cg * 8;
        float f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (r < R && c < C) {
            const float* sp = m.src + (size_t)r * C + c;
            const float4 a = *reinterpret_cast<const float4*>(sp), bb = *reinterpret_cast<const float4*>(sp + 4);
            f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = bb.x; f[5] = bb.y; f[6] = bb.z; f[7] = bb.w;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) tile[rl + 32 * p][cg * 8 + k] = f[k];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int c = c0 + rl + 32 * p, r = r0 + cg * 8;       // output row = source column c, 8 consecutive source rows
        if (c < C && r < R) {
            float f[8];
#pragma unroll
            for (int k = 0; k < 8; k++) f[k] = tile[cg * 8 + k][rl + 32 * p];
            uint4 hi, lo;
            x3_pair8(f, hi, lo);
            x3_store(m.dst + (size_t)c * 3 * R, R, r, m.form, hi, lo);
        }
    }
}
int x3_split_multi(const X3SplitBatch& b, hipStream_t st) {
    if (b.n <= 0) return CC_OK;
    int mr = 0, mc = 0;
    for (int i = 0; i < b.n; i++) {
        if ((b.it[i].R & 7) || (b.it[i].C & 7)) return CC_ERR_SHAPE;
        mr = std::max(mr, b.it[i].R);
        mc = std::max(mc, b.it[i].C);
    }
    hipLaunchKernelGGL(k_x3_split_multi, dim3((mc + 63) / 64, (mr + 63) / 64, b.n), dim3(256), 0, st, b);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

const op16_t* x3_operand(Call& cx, const float* src, size_t ld, int rows, int width, int form, bool first, int* rc) {
    if (first) cx.x3_used = 0;
    const size_t need = (((size_t)rows * 3 * width * sizeof(op16_t)) + 255) & ~size_t(255);
    if (!cx.x3 || cx.x3_used + need > cx.x3_bytes) { *rc = CC_ERR_STATE; return nullptr; }
    op16_t* dst = reinterpret_cast<op16_t*>(cx.x3 + cx.x3_used);
    cx.x3_used += need;
    *rc = x3_split_rows(src, ld, dst, rows, width, form, cx.st);
    return *rc == CC_OK ? dst : nullptr;
}
#endif   // CC_OP == 2

}  // namespace CC_NS
