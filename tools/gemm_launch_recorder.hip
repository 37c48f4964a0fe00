// Driver of the GEMM launch recorder (tools/record_gemm_launches.py builds and runs it; see there).  Built host-only together with a tree's
// gemm_inst_*.hip, tools/gemm_launch_hook.h force-included: it calls the public GEMM wrappers of gemm_api.h over a fixed list of cases and
// prints, per case, the return status and every launch the wrappers made (kernel stub address, grid, block, LDS bytes, GemmShape fields,
// integer arguments).  One process = one setting of the mode globals' defaults and of the lab switches (they are read once per process);
// the mode globals themselves are varied here.  Usage: gemm_launch_recorder core|full
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include "gemm_api.h"

namespace cc_shared {
int g_gemm_tile_mode = -1, g_gemm_s64 = -1, g_gemm_small_x2 = 1, g_decode_last_path = 0;
Prof g_prof;
}  // namespace cc_shared
namespace cc_rec {
std::vector<Launch>& log() { static std::vector<Launch> v; return v; }
}  // namespace cc_rec
extern "C" void cc_rec_anchor() {}

namespace CC_NS {
alignas(256) static char g_buf[4096];
#if CC_OP == 2
// adapter: the operand split lives in another unit; the launchers only test the image pointer for alignment
const op16_t* x3_operand(Call&, const float*, size_t, int, int, int, bool, int*) { return reinterpret_cast<const op16_t*>(g_buf); }
#endif
static bool g_full = false;
static std::set<std::string> g_seen;      // a case that two lists name is recorded once per pass

template <class F> static void rec(const std::string& id, F&& f) {
    if (!g_seen.insert(id).second) return;
    cc_rec::log().clear();
    const int rc = f();
    printf("{\"id\":\"%s\",\"rc\":%d,\"L\":[", id.c_str(), rc);
    bool first = true;
    for (const auto& l : cc_rec::log()) {
        printf("%s{\"k\":%lld,\"g\":[%u,%u,%u],\"b\":[%u,%u,%u],\"lds\":%zu,\"s\":[", first ? "" : ",", (long long)((intptr_t)l.stub - (intptr_t)&cc_rec_anchor),
               l.grid[0], l.grid[1], l.grid[2], l.block[0], l.block[1], l.block[2], l.lds);
        for (size_t i = 0; i < l.shapes.size(); i++) printf("%s%lld", i ? "," : "", l.shapes[i]);
        printf("],\"i\":[");
        for (size_t i = 0; i < l.ints.size(); i++) printf("%s%lld", i ? "," : "", l.ints[i]);
        printf("]}");
        first = false;
    }
    printf("]}\n");
}
static std::string S(std::initializer_list<long long> v) {
    std::string s;
    for (long long x : v) { s += s.empty() ? "" : ","; s += std::to_string(x); }
    return s;
}

template <class T> static T* P(int misalign = 0) { return reinterpret_cast<T*>(g_buf + 256 + misalign * (int)sizeof(T)); }
static ActIn AIN(int K, int mis = 0) { return ActIn(P<const act_t>(mis), kX3 ? K : 0); }
static Call g_cx;

// ---- the wrappers, one recorded call each -------------------------------------------------------------------------------------
static void bf16out(int al, int bl, int M, int N, int K, int lda, int ldb, int ldc, bool bias, int act, bool pre, int cimg = 0, int mis = 0) {
    rec("bf16out:" + S({al, bl, M, N, K, lda, ldb, ldc, bias, act, pre, cimg, mis}), [&] {
        return gemm_bf16out(al, bl, AIN(K, mis), lda, P<const op16_t>(), ldb, M, N, K, Act(P<act_t>(), cimg), ldc, bias ? P<const float>() : nullptr, act,
                            pre ? P<act_t>() : nullptr, g_cx);
    });
}
static void resid(int al, int bl, int M, int N, int K, int lda, int ldb, int ld, bool drop) {
    rec("resid:" + S({al, bl, M, N, K, lda, ldb, ld, drop}), [&] {
        Drop d;
        if (drop) d.thresh = 1000;
        return gemm_resid(al, bl, AIN(K), lda, P<const op16_t>(), ldb, M, N, K, P<float>(), P<const float>(), ld, P<const float>(), g_cx, d);
    });
}
static void f32out(int al, int bl, int M, int N, int K, int lda, int ldb, int ldc, int mode, int ksplit, int mis = 0) {
    rec("f32out:" + S({al, bl, M, N, K, lda, ldb, ldc, mode, ksplit, mis}), [&] {
        return gemm_f32out(al, bl, AIN(K), lda, P<const op16_t>(mis), ldb, M, N, K, P<float>(), ldc, mode == 0 ? P<const float>() : nullptr, mode, 1.0f, ksplit, g_cx);
    });
}
static void dact(int M, int N, int K, int act, int cimg = 0, int al = 0, int bl = 0) {
    rec("dact:" + S({M, N, K, act, cimg, al, bl}), [&] {
        return gemm_dact(al, bl, AIN(K), al ? M : K, P<const op16_t>(), bl ? N : K, M, N, K, Act(P<act_t>(), cimg), N, P<const act_t>(), act, g_cx);
    });
}
static void image(int N, int K) {
#ifdef CC_EXPERIMENTS
    rec("image:" + S({N, K}), [&] { return skinny_image(P<const op16_t>(), P<op16_t>(), N, K, nullptr); });
#endif
}
static void lmhead(int M, int Vp, int V, int K, int form) {      // 0 plain, 1 exponential, 2 score, 3 decode partials
    rec("lmhead:" + S({M, Vp, V, K, form}), [&] {
        const int npart = (Vp + 63) / 64;
        if (form == 0) return gemm_lmhead(AIN(K), K, P<const op16_t>(), K, M, Vp, V, K, Act(P<act_t>()), Vp, P<float>(), P<float>(), npart, P<const int>(), P<float>(), g_cx);
        if (form == 1) return gemm_lmhead(AIN(K), K, P<const op16_t>(), K, M, Vp, V, K, Act(P<act_t>()), Vp, P<float>(), P<float>(), npart, P<const int>(), P<float>(), g_cx, P<const float>());
        if (form == 2) return gemm_lmhead_score(AIN(K), K, P<const op16_t>(), K, M, Vp, V, K, P<float>(), P<float>(), npart, P<const int>(), P<float>(), g_cx);
        return gemm_logits_part(AIN(K), K, P<const op16_t>(), K, M, Vp, V, K, P<float>(), Vp, P<float>(), P<float>(), npart, g_cx);
    });
}
static void skinny(int M, int N, int K, int act, bool res, int out, int fuse, long long scratch_slabs_x4, bool bimg = false, int lda = 0) {
    // out: 16 or 32; fuse: 0 none, 1 LayerNorm, 2 KV append; scratch in quarter slabs (-1: none)
    rec("skinny:" + S({M, N, K, act, res, out, fuse, scratch_slabs_x4, bimg, lda}), [&] {
        SkinnyFuse f;
        if (fuse == 1) { f.ln_gamma = P<const float>(); f.ln_beta = P<const float>(); f.ln_out16 = P<act_t>(); }
        if (fuse == 2) { f.kcache = P<act_t>(); f.vcache = P<act_t>(); f.ctx_max = 80; }
        if (bimg) f.bimg = P<const op16_t>();
        const size_t bytes = scratch_slabs_x4 < 0 ? 0 : (size_t)M * N * (size_t)scratch_slabs_x4;      // x4 quarter slabs of 4-byte floats
        return gemm_nt_skinny(AIN(K), lda ? lda : K, P<const op16_t>(), K, M, N, K, P<const float>(), act, res ? P<const float>() : nullptr, out == 32 || res ? P<float>() : nullptr,
                              out == 16 && !res ? P<act_t>() : nullptr, N, scratch_slabs_x4 < 0 ? nullptr : P<float>(), bytes, g_cx, (fuse || bimg) ? &f : nullptr);
    });
}
static void deepk(int M, int N, int K, bool fix, long long scratch_slabs) {
    rec("deepk:" + S({M, N, K, fix, scratch_slabs}), [&] {
        LmFix lf{P<const float>(), P<const int>(), P<const op16_t>()};
        return gemm_nt_deepk(AIN(K), K, P<const op16_t>(), K, M, N, K, P<act_t>(), N, scratch_slabs < 0 ? nullptr : P<float>(), (size_t)M * N * 4 * (size_t)(scratch_slabs < 0 ? 0 : scratch_slabs), g_cx,
                             fix ? &lf : nullptr);
    });
}
struct WG { int Mw, Nw; };
// one weight gradient on its own (batch = 0), or a batch: mode 1 = parked reduces, 2 = deferred group, 3 = deferred direct group of `cap`
static void wgrad(std::initializer_list<WG> ps, int K, int mode, bool scratch, int cap = 4, size_t used = 0, int ldx_add = 0, int mis = 0) {
    std::string id = "wgrad:" + S({K, mode, scratch, cap, (long long)used, ldx_add, mis});
    for (auto p : ps) id += ";" + S({p.Mw, p.Nw});
    rec(id, [&] {
        WgradBatch wb;
        wb.defer = mode >= 2; wb.direct = mode == 3; wb.cap = cap; wb.used = used;
        if (used) { wb.n = 1; wb.it[0] = WgradBatch::Item{P<const float>(), 1024, 1, 64, P<float>(), 64, 256}; }
        for (auto p : ps) {
            const ActIn X(P<const act_t>(mis), kX3 ? p.Mw : 0);
            const int rc = gemm_wgrad(X, p.Mw + ldx_add, P<const act_t>(), p.Nw, p.Mw, p.Nw, K, P<float>(), p.Nw, scratch ? P<float>() : nullptr, g_cx, mode ? &wb : nullptr);
            if (rc != CC_OK) return rc;
        }
        return mode ? wgrad_flush(wb, nullptr) : CC_OK;
    });
}

// ---- the case lists -----------------------------------------------------------------------------------------------------------
// what the four bench.py training configurations send (mapper forward / backward, GPT-2 forward / backward, lm_head chain)
static void product_train(int D, int E, int B, bool fullft) {
    const int P_ = 10, Mm = B * 20, Mg = B * 50, Mc = B * 40, Hm = 2 * D, PD = P_ * D, Vp = 50304, V = 50257;
    f32out(0, 0, B, PD, E, E, E, 20 * D, 0, 1);
    bf16out(0, 0, Mm, 3 * D, D, D, D, 3 * D, false, 0, false);
    resid(0, 0, Mm, D, D, D, D, D, false);
    bf16out(0, 0, Mm, Hm, D, D, D, Hm, true, 1, false);
    resid(0, 0, Mm, D, Hm, Hm, Hm, D, false);
    dact(Mm, Hm, D, 1);
    bf16out(0, 0, Mm, D, Hm, Hm, Hm, D, false, 0, false);
    bf16out(0, 0, Mm, D, D, D, D, D, false, 0, false);
    bf16out(0, 0, Mm, D, 3 * D, 3 * D, 3 * D, D, false, 0, false);
    // mapper weight gradients: all 8 layers deferred into one direct launch; one layer deferred (the bf16x3 and large-batch form); parked; alone
    wgrad({{D, Hm}, {Hm, D}, {D, D}, {3 * D, D}, {D, Hm}, {Hm, D}, {D, D}, {3 * D, D}, {D, Hm}, {Hm, D}, {D, D}, {3 * D, D}, {D, Hm}, {Hm, D}, {D, D}, {3 * D, D},
           {D, Hm}, {Hm, D}, {D, D}, {3 * D, D}, {D, Hm}, {Hm, D}, {D, D}, {3 * D, D}, {D, Hm}, {Hm, D}, {D, D}, {3 * D, D}, {D, Hm}, {Hm, D}, {D, D}, {3 * D, D}}, Mm, 3, true, 32);
    wgrad({{D, Hm}, {Hm, D}, {D, D}, {3 * D, D}}, Mm, 2, true);
    wgrad({{D, Hm}, {Hm, D}, {D, D}, {3 * D, D}}, Mm, 1, true);
    for (WG p : {WG{D, Hm}, WG{Hm, D}, WG{D, D}, WG{3 * D, D}}) wgrad({p}, Mm, 0, true);
    wgrad({{PD, E}}, B, 0, true);
    // GPT-2
    bf16out(0, 0, Mg, 3 * D, D, D, D, 3 * D, true, 0, false);
    resid(0, 0, Mg, D, D, D, D, D, false);
    resid(0, 0, Mg, D, D, D, D, D, true);
    bf16out(0, 0, Mg, 4 * D, D, D, D, 4 * D, true, 3, true);
    bf16out(0, 0, Mg, 4 * D, D, D, D, 4 * D, true, 2, false);
    bf16out(0, 0, Mg, 4 * D, D, D, D, 4 * D, true, 2, true);
    resid(0, 0, Mg, D, 4 * D, 4 * D, 4 * D, D, false);
    resid(0, 0, Mg, D, 4 * D, 4 * D, 4 * D, D, true);
    for (int form = 0; form < 3; form++) lmhead(Mc, Vp, V, D, form);
    f32out(0, 0, Mg, Vp, D, D, D, Vp, 0, 1);
    deepk(Mc, D, Vp, true, 8);
    deepk(Mc, D, Vp, false, 8);
    bf16out(0, 0, Mc, D, Vp, Vp, Vp, D, false, 0, false);
    if (kX3) bf16out(0, 0, Mc, Vp, D, D, D, Vp, true, 0, false, D);      // an output written as the next GEMM's operand image
    dact(Mg, 4 * D, D, 3);
    dact(Mg, 4 * D, D, 2);
    bf16out(0, 0, Mg, D, 4 * D, 4 * D, 4 * D, D, false, 0, false);
    bf16out(0, 0, Mg, D, D, D, D, D, false, 0, false);
    bf16out(0, 0, Mg, D, 3 * D, 3 * D, 3 * D, D, false, 0, false);
    if (fullft) {
        wgrad({{Vp, D}}, Mc, 0, true);
        wgrad({{4 * D, D}, {D, 4 * D}, {D, D}, {D, 3 * D}}, Mg, 2, true);
        for (WG p : {WG{4 * D, D}, WG{D, 4 * D}, WG{D, D}, WG{D, 3 * D}}) wgrad({p}, Mg, 0, true);
    }
}
// the decode and sampling benches: prefill of 10 rows per prefix, then one row per beam / sample
static void product_decode(int D, int M) {
    const long long big = 4 * 64;
    for (int fuse : {0, 2}) skinny(M, 3 * D, D, 0, false, 16, fuse, big);
    for (int fuse : {0, 1}) skinny(M, D, D, 0, true, 32, fuse, big);
    skinny(M, 4 * D, D, 2, false, 16, 0, big);
    for (int fuse : {0, 1}) skinny(M, D, 4 * D, 0, true, 32, fuse, big);
    lmhead(M, 50264, 50257, D, 3);
    lmhead(M, 50304, 50257, D, 3);
    f32out(0, 0, M, 50264, D, D, D, 50264, 0, 1);
}
// the edges of each rule
static void edges() {
    // operand layouts, K not a multiple of 32 / 64 / 128 / 192, M = 1, unaligned leading dimensions and pointers
    for (int K : {8, 24, 32, 64, 96, 128, 160, 192, 256, 320, 384, 576, 768, 776})
        for (int M : {1, 160, 2000}) {
            if (!g_full && (M == 160 || K == 24 || K == 320 || K == 576)) continue;
            bf16out(0, 0, M, 768, K, K, K, 768, true, 0, false);
            resid(0, 0, M, 256, K, K, K, 256, false);
            f32out(0, 0, M, 512, K, K, K, 512, 0, 1);
            dact(M, 1024, K, 3);
        }
    for (int K : {64, 100, 768})
        for (int M : {8, 300, 2048}) {
            f32out(0, 1, M, 256, K, K, 256, 256, 1, 1);
            f32out(1, 1, M, 256, K, M, 256, 256, 1, 1);
            f32out(1, 0, M, 256, K, M, K, 256, 1, 1);
            bf16out(0, 1, M, 256, K, K, 256, 256, false, 1, false);
            bf16out(1, 1, M, 256, K, M, 256, 256, false, 0, false);
            resid(0, 1, M, 256, K, K, 256, 256, false);
            resid(1, 1, M, 256, K, M, 256, 256, false);
            bf16out(0, 1, M, 256, K, K, 256, 256, false, 0, false);
            bf16out(1, 1, M, 256, K, M, 256, 256, false, 1, false);
            bf16out(0, 1, M, 256, K, K, 256, 256, true, 3, true);
            bf16out(1, 1, M, 256, K, M, 256, 256, true, 3, true);
            for (int act : {2, 3}) { dact(M, 256, K, act, 0, 0, 1); dact(M, 256, K, act, 0, 1, 1); }
        }
    // split-bf16 build: shapes whose chooser picks the 256 x 192 tile (200 tiles in one round) and a two-blocks-per-CU 128 x 128 grid, under the
    // act-3 and activation-gradient functors: with CC_X3_FUSED=0 these are the unfused forms of the kernels that have a fused one
    bf16out(0, 0, 12800, 768, 768, 768, 768, 768, true, 3, true);
    bf16out(0, 0, 5120, 1024, 768, 768, 768, 1024, true, 3, true);
    dact(12800, 768, 768, 3);
    dact(12800, 768, 768, 2);
    bf16out(0, 0, 300, 256, 104, 104, 104, 256, true, 3, true);      // the specialised functors on the register-staged kernel
    dact(300, 256, 104, 2);
    for (int form = 0; form < 4; form++) { lmhead(300, 384, 300, 104, form); lmhead(64, 384, 300, 256, form); }
    image(1024, 1024);
    image(1000, 1024);
    f32out(0, 0, 300, 256, 768, 772, 768, 256, 0, 1);     // lda % 8
    f32out(0, 0, 300, 256, 768, 768, 770, 256, 0, 1);     // ldb % 8
    f32out(0, 0, 300, 256, 768, 768, 768, 254, 0, 1);     // ldc % 4
    f32out(0, 0, 300, 252, 768, 768, 768, 256, 0, 1);     // N % 8
    f32out(0, 0, 300, 256, 768, 768, 768, 256, 0, 1, 1);  // operand pointer not 16-byte aligned
    f32out(0, 0, 0, 256, 768, 768, 768, 256, 0, 1);       // empty
    f32out(1, 1, 300, 256, 768, 300, 256, 256, 1, 1);     // M % 8 on a K-strided A
    bf16out(0, 0, 300, 256, 768, 768, 768, 252, false, 0, false);
    bf16out(0, 0, 300, 256, 768, 768, 768, 256, false, 0, false, 0, 1);
    f32out(0, 0, 300, 256, 768, 768, 768, 256, 0, 3);     // slices without the atomic mode
    // requested slice counts 1 to 9 (atomic mode), three depths
    for (int ks = 1; ks <= 9; ks++)
        for (int K : {320, 768, 5000}) {
            f32out(0, 0, 256, 512, K, K, K, 512, 2, ks);
            f32out(1, 1, 256, 512, K, 256, 512, 512, 2, ks);
        }
    // tile chooser: a sweep of grids around the round boundaries of every tile form
    for (int M : {128, 256, 640, 1280, 2560, 4000, 5120, 6400, 8192, 10240, 12800, 20480})
        for (int N : {192, 256, 768, 1024, 1536, 2304, 3072, 4096}) {
            if (!g_full && (M == 256 || M == 1280 || M == 4000 || M == 8192 || N == 256 || N == 1536)) continue;
            bf16out(0, 0, M, N, 768, 768, 768, N, true, 0, false);
            if (g_full) {
                bf16out(0, 0, M, N, 1024, 1024, 1024, N, true, 2, false);
                resid(0, 0, M, N, 768, 768, 768, N, false);
                dact(M, N, 768, 3);
                f32out(0, 0, M, N, 800, 800, 800, N, 0, 1);
            }
        }
    for (int M : {64, 640, 5120, 12800}) for (int form = 0; form < 4; form++) lmhead(M, 50304, 50257, 1024, form);
    lmhead(64, 384, 300, 128, 0);
    lmhead(64, 384, 300, 100, 3);
    // the persistent 160-row kernel's ring depths and its 32-bit offset limit
    for (int K : {192, 256, 384, 512, 576, 640, 768}) bf16out(0, 0, 12800, 768, K, K, K, 768, true, 0, false);
    bf16out(0, 0, 12800, 768, 768, 180000, 768, 768, true, 0, false);
    // skinny: scratch of 0, 1, 2, 8 slabs (and a fraction), every output kind, the fused tails, the weight image, wide N
    for (int M : {1, 64, 320, 640, 700})
        for (int N : {768, 1024, 3072, 4096}) {
            if (!g_full && (M == 640 || N == 1024)) continue;
            for (long long sl : {-1LL, 0LL, 2LL, 4LL, 8LL, 32LL}) skinny(M, N, 1024, 0, false, 16, 0, sl);
            if (g_full) {
                skinny(M, N, 1024, 1, false, 16, 0, 32);
                skinny(M, N, 4096, 2, false, 16, 0, 32);
                skinny(M, N, 1024, 0, false, 32, 0, 32);
                skinny(M, N, 4096, 0, true, 32, 1, 32);
                skinny(M, N, 1024, 0, false, 16, 2, 32);
                skinny(M, N, 1024, 0, false, 16, 0, 32, true);
                skinny(M, N, 4096, 0, false, 16, 0, 4, true);
            }
        }
    skinny(320, 1024, 1000, 0, false, 16, 0, 32);      // K % 64
    skinny(320, 1020, 1024, 0, false, 16, 0, 32);      // N % 8
    skinny(320, 1024, 1024, 0, false, 16, 1, -1);      // fusion without scratch
    skinny(320, 1024, 1024, 0, false, 16, 0, 32, false, 1028);      // lda % 8
    skinny(320, 1024, 128, 0, false, 16, 0, 32);
    skinny(320, 1024, 896, 0, false, 16, 0, 32);
    skinny(320, 4096, 1024, 2, false, 16, 0, 4);       // the 80-row form's grid
    skinny(256, 4096, 1024, 2, false, 16, 0, 4);
    skinny(320, 4096, 1024, 0, true, 32, 0, 4);
    skinny(64, 50304, 768, 0, false, 32, 0, 32);
    // the weight-image form (lab build) under every functor that reaches it
    skinny(64, 1024, 1024, 0, true, 32, 0, -1, true);
    skinny(64, 1024, 8192, 0, false, 16, 0, 32, true);
    for (int act : {0, 1, 2}) skinny(64, 1024, 1024, act, false, 16, 0, -1, true);
    skinny(2000, 768, 768, 0, false, 16, 0, 32);
    // deep K
    for (int M : {256, 5120, 10240, 40000})
        for (int N : {768, 1024, 2048})
            for (long long sl : {-1LL, 0LL, 1LL, 2LL, 8LL}) if (g_full || N != 1024) deepk(M, N, 50304, M == 5120, sl);
    deepk(10240, 768, 4096, false, 8);
    deepk(10240, 768, 50300, false, 8);
    deepk(10240, 772, 50304, false, 8);
    deepk(10240, 768, 8192, false, 8);
    deepk(10240, 768, 9216, false, 8);
    // weight gradients: the three single forms, scratch that fits 0 / 1 / 2 / 8 slabs behind parked ones, unaligned operands, batches
    for (int K : {96, 256, 1000, 1024, 5120, 12800})
        for (WG p : {WG{768, 768}, WG{768, 3072}, WG{50304, 768}, WG{136, 64}, WG{4096, 4096}}) {
            wgrad({p}, K, 0, true);
            wgrad({p}, K, 0, false);
            if (g_full) wgrad({p}, K, 1, true);
        }
    const size_t full96 = size_t(96) << 20, slab = size_t(1024) * 1024 * 4;
    for (size_t left : {slab / 2, slab, 2 * slab, 8 * slab}) wgrad({{1024, 1024}}, 12800, 1, true, 4, full96 - left);
    for (size_t left : {slab / 2, slab, 2 * slab, 8 * slab}) wgrad({{1024, 1024}}, 12800, 2, true, 4, full96 - left);
    wgrad({{768, 768}}, 5120, 0, true, 4, 0, 4);       // ldx % 8
    wgrad({{768, 768}}, 5120, 0, true, 4, 0, 0, 1);    // pointer alignment
    wgrad({{764, 768}}, 5120, 0, true);                // Mw % 8
    wgrad({{768, 764}}, 5120, 0, true);                // Nw % 8
    for (int K : {1024, 1056, 5120, 12800}) {
        wgrad({{768, 768}, {768, 1536}}, K, 2, true);
        wgrad({{768, 768}, {768, 1536}, {1536, 768}, {2304, 768}, {768, 768}}, K, 2, true);
        wgrad({{768, 768}, {768, 1536}, {1536, 768}, {2304, 768}, {768, 768}}, K, 3, true, 8);
        wgrad({{768, 768}}, K, 3, true, 8);
    }
    wgrad({{4096, 4096}, {4096, 4096}, {4096, 1024}}, 2048, 2, true);
    wgrad({{768, 768}, {768, 1536}}, 5152, 3, true, 8);     // K % 64 with K % 32 == 0: not deferred
}
static void set_modes(int tile, int s64, int x2) { cc_shared::g_gemm_tile_mode = tile; cc_shared::g_gemm_s64 = s64; cc_shared::g_gemm_small_x2 = x2; }
static void all_cases() {
    product_train(768, 512, 256, true);
    product_train(1024, 1024, 128, true);
    product_train(768, 512, 16, false);
    for (int D : {768, 1024}) for (int M : {64, 320, 640, 3200}) product_decode(D, M);
    edges();
}
}  // namespace CC_NS

int main(int argc, char** argv) {
    using namespace CC_NS;
    const bool full = argc > 1 && !strcmp(argv[1], "full");
    // the full list under the default modes, then (full only) the core list under each mode global's other values
    auto pass = [](const char* modes, int tile, int s64, int x2, bool all) {
        printf("{\"modes\":\"%s\"}\n", modes);
        set_modes(tile, s64, x2);
        g_full = all;
        g_seen.clear();
        all_cases();
    };
    pass("", -1, -1, 1, full);
    if (full) {
        char m[32];
        for (int tile : {0, 3, 4, 5, 6, 7}) { snprintf(m, sizeof m, "tile=%d", tile); pass(m, tile, -1, 1, false); }
        for (int s64 : {0, 1, 2}) { snprintf(m, sizeof m, "s64=%d", s64); pass(m, -1, s64, 1, false); }
        pass("x2=0", -1, -1, 0, false);
        pass("tile=0,s64=0,x2=0", 0, 0, 0, false);
    }
    return 0;
}
