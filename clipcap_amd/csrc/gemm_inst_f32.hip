// Built with `make ABLATION=1` this TU also carries the timing-only ablation variants of the NT kernel (CC_GEMM_ABL=1|2|4|5|6 at
// run time, tools/gemm_bench.py); the default build has none, so product code generation is not perturbed by sibling variants.
#include "gemm.hip.h"
#include <algorithm>
#include "gemm_api.h"
namespace CC_NS {
// both operands already in the 16-bit operand form (in the bf16x3 build: their hi / lo images, K = 3 x the logical depth)
static int gemm_f32out_op(int al, int bl, const op16_t* A, int lda, const op16_t* B, int ldb, int M, int N, int K, float* C, int ldc,
                          const float* bias, int mode, float alpha, int ksplit, hipStream_t st) {
    if ((ldc & 3) || (N & 7)) return CC_ERR_SHAPE;
    if (ksplit > 1 && mode != 2) return CC_ERR_ARG;  // slab mode (3) is reached through gemm_wgrad only
    EpiF32 e{C, bias, ldc, M, N, mode, alpha};
    return launch_gemm(al, bl, A, lda, B, ldb, M, N, K, ksplit, e, st);
}
int gemm_f32out(int al, int bl, ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, float* C, int ldc,
                const float* bias, int mode, float alpha, int ksplit, Call& cx) {
    const hipStream_t st = cx.st;
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, 2.0 * M * N * (double)K);
    const op16_t* A16;
    const int rca = nt_operand(cx, A, al, bl, M, lda, ldb, K, A16);
    if (rca != CC_OK) return rca;
    return gemm_f32out_op(al, bl, A16, lda, B, ldb, M, N, K, C, ldc, bias, mode, alpha, ksplit, st);
}
__global__ __launch_bounds__(256) void k_slab_reduce(const float* __restrict__ slabs, size_t slab_elems, int ks, int Nw, float* __restrict__ dW,
                                                     int ldw, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 a = reinterpret_cast<const float4*>(slabs)[i];
        for (int s = 1; s < ks; s++) {
            const float4 b = reinterpret_cast<const float4*>(slabs + s * slab_elems)[i];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        const size_t e = i * 4;
        float* d = dW + (e / Nw) * ldw + (e % Nw);
        const float4 c = *reinterpret_cast<const float4*>(d);
        *reinterpret_cast<float4*>(d) = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    }
}

struct SlabItems { WgradBatch::Item it[8]; };
__global__ __launch_bounds__(256) void k_slab_reduce_multi(SlabItems items) {
    const WgradBatch::Item& q = items.it[blockIdx.y];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < q.n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 a = reinterpret_cast<const float4*>(q.slabs)[i];
        for (int s = 1; s < q.ks; s++) {
            const float4 b = reinterpret_cast<const float4*>(q.slabs + s * q.slab)[i];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        const size_t e = i * 4;
        float* d = q.dW + (e / q.Nw) * q.ldw + (e % q.Nw);
        const float4 c = *reinterpret_cast<const float4*>(d);
        *reinterpret_cast<float4*>(d) = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    }
}
// the deferred problems of a batch as one grouped launch (cc_plan::plan_wgrad_group_direct / plan_wgrad_group); the slab form's slabs are
// parked for the batched reduce
static int wgrad_launch_group(WgradBatch& b, hipStream_t st) {
    if (b.nd == 0) return CC_OK;
    const int K = b.d[0].K;
    double flops = 0.0;
    cc_plan::WgradProblem pr[TT_GROUP_MAX];
    for (int i = 0; i < b.nd; i++) { pr[i] = {b.d[i].Mw, b.d[i].Nw}; flops += 2.0 * b.d[i].Mw * b.d[i].Nw * (double)K; }
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, flops);
    const cc_plan::WgradGroupPlan p = b.direct ? cc_plan::plan_wgrad_group_direct(pr, b.nd, K, b.scratch && b.n == 0, WGRAD_SCRATCH_BYTES, cc_plan::gemm_knobs())
                                               : cc_plan::plan_wgrad_group(pr, b.nd, K, WGRAD_SCRATCH_BYTES - b.used, cc_plan::gemm_knobs());
    if (p.status != CC_OK) return p.status;
    TTGroup grp;
    grp.n = b.nd;
    grp.mode = b.direct ? 1 : 0;
    if (p.whole >= 0) { grp.whole = p.whole; grp.split = p.split; grp.tail = b.scratch; }
    for (int i = 0; i < b.nd; i++) {
        const auto& d = b.d[i];
        grp.A[i] = d.X; grp.B[i] = d.Y;
        grp.g[i] = GemmShape{d.Mw, d.Nw, d.K, d.ldx, d.ldy, p.k_chunk, 8, 0};
        if (b.direct) {      // dW += tile in the epilogue
            grp.slab[i] = d.dW; grp.zstride[i] = 0; grp.ldc[i] = d.ldw;
        } else {
            const size_t slab = (size_t)d.Mw * d.Nw;
            float* sc = b.scratch + b.used / sizeof(float);
            grp.slab[i] = sc; grp.zstride[i] = slab; grp.ldc[i] = d.Nw;
            b.it[b.n++] = WgradBatch::Item{sc, slab, p.ks, d.Nw, d.dW, d.ldw, slab / 4};
            b.used += (size_t)p.ks * slab * sizeof(float);
            b.used = (b.used + 255) & ~size_t(255);
        }
    }
    for (int i = 0; i <= TT_GROUP_MAX; i++) grp.first[i] = p.first[i];
    b.nd = 0;
    return launch_gemm_tt_group(grp, p, st);
}

int wgrad_flush(WgradBatch& b, hipStream_t st) {
    const int rcg = wgrad_launch_group(b, st);
    if (rcg != CC_OK) return rcg;
    if (b.n == 0) return CC_OK;
    SlabItems items;
    size_t nmax = 0;
    for (int i = 0; i < b.n; i++) { items.it[i] = b.it[i]; nmax = std::max(nmax, b.it[i].n4); }
    hipLaunchKernelGGL(k_slab_reduce_multi, dim3((int)std::min<size_t>((nmax + 255) / 256, 1024), b.n), dim3(256), 0, st, items);
    b.n = 0;
    b.used = 0;
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}
// folds `ks` slabs at `slabs` into dW: immediately, or parked in the batch
static int wgrad_reduce(const float* slabs, size_t slab, int ks, int Nw, float* dW, int ldw, WgradBatch* batch, hipStream_t st) {
    const size_t n4 = slab / 4;
    if (batch) {
        batch->it[batch->n++] = WgradBatch::Item{slabs, slab, ks, Nw, dW, ldw, n4};
        batch->used += (size_t)ks * slab * sizeof(float);
        batch->used = (batch->used + 255) & ~size_t(255);
        if (batch->n == 8) return wgrad_flush(*batch, st);
        return CC_OK;
    }
    hipLaunchKernelGGL(k_slab_reduce, dim3((int)std::min<size_t>((n4 + 255) / 256, 2048)), dim3(256), 0, st, slabs, slab, ks, Nw, dW, ldw, n4);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

int gemm_wgrad(ActIn Xa, int ldx, const act_t* Ya, int ldy, int Mw, int Nw, int K, float* dW, int ldw, float* scratch,
               Call& cx, WgradBatch* batch) {
    const hipStream_t st = cx.st;
    if ((Nw & 7) || (ldw & 3)) return CC_ERR_SHAPE;
    const double flops = 2.0 * Mw * Nw * (double)K;
#if CC_OP == 2
    // bf16x3: dW = X^T Y = Xhi^T Yhi + Xhi^T Ylo + Xlo^T Yhi.  The [K][3 Mw] image [hi | hi | lo] of X, read as a [3K][Mw] matrix, has
    // rows (hi, hi, lo) per source row, the [hi | lo | hi] image of Y rows (hi, lo, hi): the unchanged kernels contract over K' = 3K.
    // The images live in the call's scratch, so nothing can be deferred to a grouped launch.
    if (Mw & 7) return CC_ERR_SHAPE;
    if (Xa.img && Xa.img != Mw) return CC_ERR_ARG;
    int rcx = CC_OK;
    // the first operand (the output gradient) has the [hi | hi | lo] form the input-gradient GEMM of the same tensor reads as its A operand:
    // a caller that has split it once for both passes that image
    const bool ximg = Xa.img != 0;
    const op16_t* X = ximg ? reinterpret_cast<const op16_t*>(Xa.p) : x3_operand(cx, Xa.p, (size_t)ldx, K, Mw, 0, true, &rcx);
    if (!X) return rcx;
    const op16_t* Y = x3_operand(cx, Ya, (size_t)ldy, K, Nw, 1, ximg, &rcx);
    if (!Y) return rcx;
    ldx = Mw; ldy = Nw; K *= 3;
    const bool may_defer = false;
#else
    if (Xa.img) return CC_ERR_ARG;
    const op16_t* X = Xa.p;
    const op16_t* Y = Ya;
    const bool may_defer = true;
#endif
    const size_t slab = (size_t)Mw * Nw;
    // the DMA-staged TT kernels need 16-B aligned operands and row strides; anything else takes the register-staged kernel
    const bool tt_ok = (Mw & 7) == 0 && (ldx & 7) == 0 && (ldy & 7) == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)Y & 15) == 0;
    // scratch left behind the batch's parked slabs; a gradient that cannot get at least 2 slices there flushes the batch first
    if (batch && scratch && batch->n > 0 && WGRAD_SCRATCH_BYTES - batch->used < 2 * slab * sizeof(float)) {
        const int rcf = wgrad_flush(*batch, st);
        if (rcf != CC_OK) return rcf;
    }
    // grouped path: park the problem; wgrad_flush launches the layer's gradients together (one tail, one launch floor)
    // a deferred problem needs at least one slab behind the parked ones and the other deferred problems' slabs (wgrad_launch_group then
    // finds a slice count that fits); a gradient whose single slab exceeds the scratch (GPT-2-xl width: c_fc 4 D^2 fp32 = 41 MB is fine,
    // but 12 D^2 = 123 MB for the layer is not) makes the group flush early, one larger than the whole scratch is never deferred
    const size_t slab_bytes = ((slab * sizeof(float)) + 255) & ~size_t(255);
    if (may_defer && batch && batch->defer && g_gemm_tile_mode != 0 && tt_ok && scratch && (K % G_BK) == 0 && K >= 1024 && (slab & 3) == 0 &&
        slab_bytes <= WGRAD_SCRATCH_BYTES && (batch->nd == 0 || batch->d[0].K == K)) {
        size_t pending = 0;
        for (int i = 0; i < batch->nd; i++) pending += (((size_t)batch->d[i].Mw * batch->d[i].Nw * sizeof(float)) + 255) & ~size_t(255);
        const int cap = std::min(std::max(batch->cap, 1), 32);
        if (batch->nd == cap || (!batch->direct && (batch->n + batch->nd >= 8 || batch->used + pending + slab_bytes > WGRAD_SCRATCH_BYTES))) {
            const int rcf = wgrad_flush(*batch, st);
            if (rcf != CC_OK) return rcf;
        }
        batch->scratch = scratch;
        batch->d[batch->nd++] = WgradBatch::Deferred{X, Y, ldx, ldy, Mw, Nw, K, dW, ldw};
        return CC_OK;
    }
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, flops);
    const size_t used = (batch && scratch) ? batch->used : 0;
    float* sc = scratch ? scratch + used / sizeof(float) : nullptr;
    const cc_plan::WgradPlan p = cc_plan::plan_wgrad(Mw, Nw, K, tt_ok, scratch != nullptr, WGRAD_SCRATCH_BYTES - used, gemm_modes());
    if (p.form == cc_plan::WG_TT256_DIRECT) {
        EpiF32 e{dW, nullptr, ldw, Mw, Nw, 1, 1.0f};
        return launch_gemm_tt<256>(X, ldx, Y, ldy, Mw, Nw, K, 1, e, nullptr, st);
    }
    if (p.form == cc_plan::WG_REG_DIRECT) return gemm_f32out_op(1, 1, X, ldx, Y, ldy, Mw, Nw, K, dW, ldw, nullptr, 1, 1.0f, 1, st);
    // slices z write slab z (EpiF32 store mode; C pointer advanced per z inside the kernel via blockIdx.z * slab)
    EpiF32 e{sc, nullptr, Nw, Mw, Nw, 3, 1.0f};
    e.zstride = slab;
    int ks_eff = 1;
    const int rc = p.form == cc_plan::WG_TT256_SLABS   ? launch_gemm_tt<256>(X, ldx, Y, ldy, Mw, Nw, K, p.ks, e, &ks_eff, st)
                   : p.form == cc_plan::WG_TT128_SLABS ? launch_gemm_tt<128>(X, ldx, Y, ldy, Mw, Nw, K, p.ks, e, &ks_eff, st)
                                                       : launch_gemm(1, 1, X, ldx, Y, ldy, Mw, Nw, K, p.ks, e, st, -2, 0, &ks_eff);
    if (rc != CC_OK) return rc;
    return wgrad_reduce(sc, slab, ks_eff, Nw, dW, ldw, batch, st);
}

__global__ __launch_bounds__(256) void k_splitk_finish(const float* __restrict__ slabs, size_t slab_elems, int ks, int M, int N,
                                                       const float* __restrict__ bias, int act, const float* __restrict__ res,
                                                       float* __restrict__ out32, act_t* __restrict__ out16, int ldo) {
    const size_t n8 = (size_t)M * (N >> 3);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / (N >> 3)), col = (int)(i % (N >> 3)) * 8;
        const size_t e = (size_t)row * N + col;
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int s = 0; s < ks; s++) {
            const float4 a = *reinterpret_cast<const float4*>(slabs + s * slab_elems + e);
            const float4 b = *reinterpret_cast<const float4*>(slabs + s * slab_elems + e + 4);
            v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
        }
        if (bias) {
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] += bias[col + k];
        }
        if (act == 1) {
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = fmaxf(v[k], 0.f);
        } else if (act == 2) {
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = gelu_new_f(v[k]);
        }
        const size_t o = (size_t)row * ldo + col;
        if (res) {
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] += res[o + k];
        }
        if (out32) {
            *reinterpret_cast<float4*>(out32 + o) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(out32 + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
        if (out16) act_st8(out16 + o, v);
    }
}

// one 256-thread block per finished row (M is small here, so rows are the only parallelism): slabs -> (+bias, act, +residual) ->
// fp32 / bf16 stores -> optional KV append -> optional LayerNorm (block reduction) -> bf16
__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(256) void k_splitk_finish_row(const float* __restrict__ slabs, size_t slab_elems, int ks, int M, int N,
                                                           const float* __restrict__ bias, int act, const float* __restrict__ res,
                                                           float* __restrict__ out32, act_t* __restrict__ out16, int ldo, SkinnyFuse f) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    constexpr int MAXV = 3;                // float4 per thread -> N <= 3072
    float4 v[MAXV];
    float s1 = 0.f;
    // LayerNorm parameters are fetched up front, beside the slab loads, not after the two block reductions
    float4 lg_[MAXV], lb_[MAXV];
    if (f.ln_out16) {
#pragma unroll
        for (int it = 0; it < MAXV; it++) {
            const int c = threadIdx.x * 4 + it * 1024;
            if (c < N) { lg_[it] = *reinterpret_cast<const float4*>(f.ln_gamma + c); lb_[it] = *reinterpret_cast<const float4*>(f.ln_beta + c); }
        }
    }
#pragma unroll
    for (int it = 0; it < MAXV; it++) {
        const int c = threadIdx.x * 4 + it * 1024;
        if (c < N) {
            float4 a = make_float4(0, 0, 0, 0);
            const float* sp = slabs + (size_t)row * N + c;
            float4 bb = make_float4(0, 0, 0, 0), rr = make_float4(0, 0, 0, 0);
            if (bias) bb = *reinterpret_cast<const float4*>(bias + c);
            if (res) rr = *reinterpret_cast<const float4*>(res + (size_t)row * ldo + c);
            int s = 0;
            for (; s + 4 <= ks; s += 4) {                      // four slices in flight
                const float4 p0 = *reinterpret_cast<const float4*>(sp + (s + 0) * slab_elems), p1 = *reinterpret_cast<const float4*>(sp + (s + 1) * slab_elems);
                const float4 p2 = *reinterpret_cast<const float4*>(sp + (s + 2) * slab_elems), p3 = *reinterpret_cast<const float4*>(sp + (s + 3) * slab_elems);
                a.x += (p0.x + p1.x) + (p2.x + p3.x); a.y += (p0.y + p1.y) + (p2.y + p3.y);
                a.z += (p0.z + p1.z) + (p2.z + p3.z); a.w += (p0.w + p1.w) + (p2.w + p3.w);
            }
            if (ks - s == 3) {
                const float4 p0 = *reinterpret_cast<const float4*>(sp + (s + 0) * slab_elems), p1 = *reinterpret_cast<const float4*>(sp + (s + 1) * slab_elems);
                const float4 p2 = *reinterpret_cast<const float4*>(sp + (s + 2) * slab_elems);
                a.x += (p0.x + p1.x) + p2.x; a.y += (p0.y + p1.y) + p2.y; a.z += (p0.z + p1.z) + p2.z; a.w += (p0.w + p1.w) + p2.w;
            } else {
                for (; s < ks; s++) {
                    const float4 p = *reinterpret_cast<const float4*>(sp + s * slab_elems);
                    a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
                }
            }
            a.x += bb.x; a.y += bb.y; a.z += bb.z; a.w += bb.w;
            if (act == 2) { a.x = gelu_new_f(a.x); a.y = gelu_new_f(a.y); a.z = gelu_new_f(a.z); a.w = gelu_new_f(a.w); }
            else if (act == 1) { a.x = fmaxf(a.x, 0.f); a.y = fmaxf(a.y, 0.f); a.z = fmaxf(a.z, 0.f); a.w = fmaxf(a.w, 0.f); }
            const size_t o = (size_t)row * ldo + c;
            a.x += rr.x; a.y += rr.y; a.z += rr.z; a.w += rr.w;
            if (out32) *reinterpret_cast<float4*>(out32 + o) = a;
            const act_raw4 pk = act_pack4(a.x, a.y, a.z, a.w);
            if (out16) act_straw4(out16 + o, pk);
            if (f.kcache) {                   // N == 3*D
                const int D = N / 3, which = c / D, cc_ = c - which * D;
                if (which > 0) {
                    const int r = row / f.Tn, t = row - r * f.Tn;
                    act_t* dst = (which == 1 ? f.kcache : f.vcache) + ((size_t)r * f.ctx_max + f.pos0 + t) * D + cc_;
                    act_straw4(dst, pk);
                }
            }
            v[it] = a;
            s1 += a.x + a.y + a.z + a.w;
        }
    }
    if (!f.ln_out16) return;               // block-uniform
    const float mu = block_sum256(s1, red) / N;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < MAXV; it++) {
        const int c = threadIdx.x * 4 + it * 1024;
        if (c < N) { const float a = v[it].x - mu, b = v[it].y - mu, c2 = v[it].z - mu, d = v[it].w - mu; q += a * a + b * b + c2 * c2 + d * d; }
    }
    const float rs = rsqrtf(block_sum256(q, red) / N + 1e-5f);
#pragma unroll
    for (int it = 0; it < MAXV; it++) {
        const int c = threadIdx.x * 4 + it * 1024;
        if (c < N) {
            const float4 g = lg_[it], b = lb_[it];
            act_st4(f.ln_out16 + (size_t)row * N + c, (v[it].x - mu) * rs * g.x + b.x, (v[it].y - mu) * rs * g.y + b.y,
                    (v[it].z - mu) * rs * g.z + b.z, (v[it].w - mu) * rs * g.w + b.w);
        }
    }
}

int skinny_single_min_tiles() { return cc_plan::gemm_knobs().skinny_single; }
bool gemm_nt_skinny_can_fuse(int M, int N, int K, size_t scratch_bytes) {
    return M > 0 && N > 0 && (N & 7) == 0 && N <= 3072 && (K % G_BK) == 0 && scratch_bytes >= (size_t)M * N * sizeof(float);
}

// slab sum of the K-sliced lm_head input gradient in the exponential form: out = r * sum(slabs) - w * wte[target]
__global__ __launch_bounds__(256) void k_deepk_finish_lm(const float* __restrict__ slabs, size_t slab_elems, int ks, int M, int N, LmFix f,
                                                         act_t* __restrict__ out16, int ldo) {
    const size_t n8 = (size_t)M * (N >> 3);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / (N >> 3)), col = (int)(i % (N >> 3)) * 8;
        const size_t e = (size_t)row * N + col;
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b[8];
        for (int s = 0; s < ks; s++) {
            const float4 a = *reinterpret_cast<const float4*>(slabs + s * slab_elems + e);
            const float4 c = *reinterpret_cast<const float4*>(slabs + s * slab_elems + e + 4);
            v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += c.x; v[5] += c.y; v[6] += c.z; v[7] += c.w;
        }
        const float r = f.fac[2 * row], w = f.fac[2 * row + 1];
#if CC_OP == 2
        act_ld8(reinterpret_cast<const float*>(f.wte) + (size_t)f.target[row] * N + col, b);      // bf16x3: LmFix.wte is the fp32 master
#else
        unpack8(*reinterpret_cast<const uint4*>(f.wte + (size_t)f.target[row] * N + col), b);
#endif
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = r * v[k] - w * b[k];
        act_st8(out16 + (size_t)row * ldo + col, v);
    }
}

int gemm_nt_deepk(ActIn Aa, int lda, const op16_t* B, int ldb, int M, int N, int K, act_t* out16, int ldo, float* scratch,
                  size_t scratch_bytes, Call& cx, const LmFix* fix) {
    const hipStream_t st = cx.st;
    const cc_plan::DeepKPlan p = cc_plan::plan_deepk(M, N, K, lda, ldb, ldo, scratch != nullptr, scratch_bytes, gemm_modes(), cc_plan::gemm_knobs());
    if (p.status != CC_OK) return p.status;
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, 2.0 * M * N * (double)K);
    const op16_t* A;
    const int rca = nt_operand(cx, Aa, 0, 0, M, lda, ldb, K, A);
    if (rca != CC_OK) return rca;
    // (the split-bf16 slice search's refusal: kept apart from p.status so that, as before, an operand error is reported ahead of it)
    if (p.status_late != CC_OK) return p.status_late;
    const size_t slab = (size_t)M * N;
    EpiF32 e{scratch, nullptr, N, M, N, 3, 1.0f};
    e.zstride = slab;
    int ks_eff = 1;
    const int rc = launch_gemm(0, 0, A, lda, B, ldb, M, N, K, p.ks, e, st, p.tile, p.group_m, &ks_eff);
    if (rc != CC_OK) return rc;
    const size_t n8 = (size_t)M * (N >> 3);
    if (fix)
        hipLaunchKernelGGL(k_deepk_finish_lm, dim3((int)std::min<size_t>((n8 + 255) / 256, 2048)), dim3(256), 0, st, scratch, slab, ks_eff, M, N, *fix,
                           out16, ldo);
    else
        hipLaunchKernelGGL(k_splitk_finish, dim3((int)std::min<size_t>((n8 + 255) / 256, 2048)), dim3(256), 0, st, scratch, slab, ks_eff, M, N, nullptr, 0,
                           nullptr, nullptr, out16, ldo);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}

#ifdef CC_EXPERIMENTS
int skinny_image(const op16_t* W, op16_t* img, int N, int K, hipStream_t st) {
    if ((N % 64) || (K % 64) || !W || !img) return CC_ERR_SHAPE;
    hipLaunchKernelGGL(k_skinny_image, dim3(1024), dim3(256), 0, st, W, img, N, K);
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}
#endif

int gemm_nt_skinny(ActIn Aa, int lda, const op16_t* B, int ldb, int M, int N, int K, const float* bias, int act, const float* res,
                   float* out32, act_t* out16, int ldo, float* scratch, size_t scratch_bytes, Call& cx, const SkinnyFuse* fuse) {
    const hipStream_t st = cx.st;
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, 2.0 * M * N * (double)K);
    if ((N & 7) || (ldo & 7)) return CC_ERR_SHAPE;
    const op16_t* A;
    const int rca = nt_operand(cx, Aa, 0, 0, M, lda, ldb, K, A);
    if (rca != CC_OK) return rca;
    const size_t slab = (size_t)M * N;
    const bool fused = fuse && (fuse->ln_out16 || fuse->kcache);
    const op16_t* bimg = (fuse && !kX3) ? fuse->bimg : nullptr;
    const cc_plan::SkinnyPlan p = cc_plan::plan_skinny(M, N, K, lda, ldb, scratch != nullptr, scratch_bytes, fused, res != nullptr, out16 != nullptr, act,
                                                       gemm_modes(), cc_plan::gemm_knobs());
    if (p.status != CC_OK) return p.status;
    // one GEMM launch with functor e: on the 64-row kernels in the plan's form, else through the NT launcher
    // (the two functors without run-time switches exist on the 64-row kernels only)
    int ks_eff = 1;
    auto run64 = [&](const auto& e) { return launch_gemm_s64(A, lda, B, ldb, M, N, K, p.ks, p.form, e, &ks_eff, st, bimg); };
    auto run = [&](const auto& e) { return p.s64 ? run64(e) : launch_gemm(0, 0, A, lda, B, ldb, M, N, K, p.ks, e, st, -2, 0, &ks_eff); };
    if (!p.slab) {
        switch (p.functor) {
        case cc_plan::SK_RESID: return run(EpiResid{out32, res, bias, ldo, M, N});
        case cc_plan::SK_PLAIN: return run64(EpiBF16Plain{out16, bias, ldo, M, N});
        case cc_plan::SK_GELU: return run64(EpiBF16T<2, 0>{out16, nullptr, bias, ldo, M, N, 2});
        case cc_plan::SK_BF16: return run(EpiBF16{out16, nullptr, bias, ldo, M, N, act});
        default: return run(EpiF32{out32, bias, ldo, M, N, 0, 1.0f});
        }
    }
    EpiF32 e{scratch, nullptr, N, M, N, 3, 1.0f};
    e.zstride = slab;
    const int rc = run(e);
    if (rc != CC_OK) return rc;
    if (p.finish == cc_plan::FIN_REFUSE) return CC_ERR_SHAPE;
    if (p.finish == cc_plan::FIN_ROW) {
        SkinnyFuse f = fuse ? *fuse : SkinnyFuse{};
        hipLaunchKernelGGL(k_splitk_finish_row, dim3(M), dim3(256), 0, st, scratch, slab, ks_eff, M, N, bias, act, res, out32, out16, ldo, f);
    } else {
        const size_t n8 = (size_t)M * (N >> 3);
        hipLaunchKernelGGL(k_splitk_finish, dim3((int)std::min<size_t>((n8 + 255) / 256, 2048)), dim3(256), 0, st, scratch, slab, ks_eff, M, N, bias,
                           act, res, out32, out16, ldo);
    }
    return hipGetLastError() == hipSuccess ? CC_OK : CC_ERR_LAUNCH;
}
}  // namespace CC_NS
