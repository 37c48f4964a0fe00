// Deterministic cross-block reductions for gfx950: per-block partials in the call's scratch, folded in one fixed order (batch sums,
// column sums, the fold that LayerNorm backward shares) and the token-indexed scatter-add.  No atomics anywhere.
#include "kernels.h"

namespace CC_NS {

// ---- deterministic cross-block reductions (kernels.h): per-block partials in the call's scratch, folded in a fixed order ----

// partials part[y][s][j] (y < gridDim.y groups of S slices x n columns): out[y * k + j / m][j % m] += sum over s of part[y][s][j], the
// slices summed in one fixed order: per chunk of 256 slices, lane g (of 16) of a column loads s = g, g + 16, ..., g + 240 at once and adds
// them as a fixed tree; the 16 lane sums are then added in lane order.
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
int fold_partials(const float* part, int S, int n, int groups, const FoldOut& o, hipStream_t st) {
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

// ------------------------------------------------------------------------------------------------------------
// Column sums of a bf16 matrix (bias gradients): out[n] += sum_m X[m][n].  Block = 64 columns x a row slice.
// ------------------------------------------------------------------------------------------------------------
// Up to 32 equally shaped matrices in one launch (blockIdx.z = matrix): the mapper backward's per-layer fc1.bias gradients, deferred to
// the end of the call together with the weight gradients (round 5).  With more than one slice, slice y of matrix z leaves its sums in
// row z * slices + y of `part`, folded in a fixed order by k_fold_partials.
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
    ColsumBatch b;      // one matrix = a batch of one: the same slices, partial rows and fold
    b.add(X, out);
    return colsum_bf16_multi(b, ld, M, N, cx);
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
    const dim3 sum_blocks = flat_grid((size_t)R * ncb, 4, 4096);
    if (s.act) hipLaunchKernelGGL(k_sc_sum<true>, sum_blocks, dim3(256), 0, st, s, w.skeys, w.info, w.heads, w.cnt, D, ncb, dst, w.part);
    else hipLaunchKernelGGL(k_sc_sum<false>, sum_blocks, dim3(256), 0, st, s, w.skeys, w.info, w.heads, w.cnt, D, ncb, dst, w.part);
    if (R > SCATTER_CHUNK) {
        const dim3 fold_blocks = flat_grid((size_t)(R / (SCATTER_CHUNK + 1) + 1) * ncb, 4, 1024);
        hipLaunchKernelGGL(k_sc_fold, fold_blocks, dim3(256), 0, st, w.skeys, w.info, w.mstarts, w.cnt, D, ncb, w.part, dst);
    }
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

}  // namespace CC_NS
