// GEMM launch plans: every decision the GEMM host launchers make (tile form, K slices, grid, LDS bytes, ordering group, functor), as pure
// host functions.  Plain C++17 with no HIP header, so the rules can be compiled, read and tested on their own (tests/test_gemm_plan.py);
// gemm.hip.h and gemm_inst_*.hip launch what a plan says and decide nothing themselves.  To see which product shapes a changed rule
// moves: tools/record_gemm_launches.py, tools/record_gemm_launches.py --compare.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>
#include "../../include/clipcap_hip.h"
#include "lab_env.h"

namespace cc_plan {

// ---- tile sizes of the kernels (gemm.hip.h takes them from here) ---------------------------------------------------------------
constexpr int G_BM = 128, G_BN = 128, G_BK = 64, G_THREADS = 256;
constexpr int G_TILE_BYTES = G_BM * G_BK * 2;  // 16 KiB per operand per buffer
constexpr int H_BM = 256, H_BN = 256, H_BK = 32, H_NS = 4, H_STAGE = (H_BM + H_BN) * H_BK * 2;   // 32 KiB per stage, 128 KiB total (5 stages = all 160 KiB measured 2-3 % slower)

// ---- K slices: the only definition -----------------------------------------------------------------------------------------------
// `want` slices over K in whole steps: every slice is k_chunk deep (a multiple of `step`), and the ceil division may need fewer slices
// than wanted to cover K — ks_eff, which is what the launch uses and what a caller folding the slices must use.
struct KSlices { int ks_eff, k_chunk; };
inline KSlices k_slices(int K, int step, int want) {
    if (want < 1) want = 1;
    const int kt = (K + step - 1) / step, per = (kt + want - 1) / want;
    return {(kt + per - 1) / per, per * step};
}

// ---- lab switches of the dispatch: frozen defaults in the product build ------------------------------------------------------------
struct GemmKnobs {
    int group_m = 0;            // CC_GROUP_M: row tiles per ordering group of every NT launch (0 = the caller's / 8)
    int stagger = 0;            // CC_GEMM_STAGGER: GemmShape::stagger (tuning knob)
    bool s160 = true;           // CC_GEMM_S160=0: the chooser never picks the 160 x 256 form
    bool q4 = true;             // CC_GEMM_Q4=0: 160 x 256 launches stay on the staggered kernel
    bool q4_last = true;        // CC_Q4_LAST=0: GemmShape::flags bit 0
    bool x3_fused = true;       // CC_X3_FUSED=0: bf16x3 build without the fused two-stage forms (A/B switch)
    bool wgrad_tail = true;     // CC_WGRAD_TAIL=0: the direct grouped weight-gradient launch keeps whole tiles only
    int wgrad_tile = 0;         // CC_WGRAD_TILE, CC_WGRAD_KS: force the grouped weight-gradient launch's tile / slice count (tuning knobs)
    int wgrad_ks = 0;
    int skinny_single = 60;     // CC_SKINNY_SINGLE: measured on config 5: 171 (never) / 165 (90) / 159 (60) / 160 (20) ms per decode batch
    bool skinny_80 = true;      // CC_SKINNY_80=0: no 80-row form
    int deepk = -1;             // CC_DEEPK: 0 = off, n > 0 = force n slices
    bool epi_spec = true;       // CC_EPI_SPEC=0: no compile-time-specialised functors
    bool epi_plain = true;      // CC_EPI_PLAIN=0: plain launches keep the general functor
    bool pre_nt = false;        // CC_PRE_NT=1: non-temporal stores of the pre-activation copy (experiment switch)
    bool resid_init = true;     // CC_RESID_INIT=0: accumulators never start from the residual (A/B switch)
    int abl = 0;                // CC_GEMM_ABL (builds with -DCC_GEMM_ABLATION only): timing-only ablation variant of the NT kernel
};
// The one place the GEMM code looks at the environment (lab build; cc_lab_env returns nothing in the product build).
inline const GemmKnobs& gemm_knobs() {
    static const GemmKnobs knobs = []() {
        GemmKnobs k;
        auto num = [](const char* name, int dflt) { const char* e = cc_lab_env(name); return e ? atoi(e) : dflt; };
        auto on = [](const char* name) { const char* e = cc_lab_env(name); return !e || atoi(e) != 0; };      // default on
        k.group_m = num("CC_GROUP_M", 0);
        k.stagger = num("CC_GEMM_STAGGER", 0);
        k.s160 = on("CC_GEMM_S160");
        k.q4 = on("CC_GEMM_Q4");
        k.q4_last = on("CC_Q4_LAST");
        k.x3_fused = on("CC_X3_FUSED");
        k.wgrad_tail = on("CC_WGRAD_TAIL");
        k.wgrad_tile = num("CC_WGRAD_TILE", 0);
        k.wgrad_ks = num("CC_WGRAD_KS", 0);
        k.skinny_single = num("CC_SKINNY_SINGLE", 60);
        k.skinny_80 = on("CC_SKINNY_80");
        k.deepk = num("CC_DEEPK", -1);
        k.epi_spec = on("CC_EPI_SPEC");
        k.epi_plain = on("CC_EPI_PLAIN");
        k.pre_nt = num("CC_PRE_NT", 0) != 0;
        k.resid_init = on("CC_RESID_INIT");
#ifdef CC_GEMM_ABLATION
        k.abl = num("CC_GEMM_ABL", 0);
#endif
        return k;
    }();
    return knobs;
}

// What the planner needs to know about the process and the build: the cc_shared::g_gemm_* mode globals (test / measurement hooks), whether
// this is the bf16x3 build, and the CU count.
struct GemmModes {
    int tile_mode;      // g_gemm_tile_mode: -1 chooser, 0 = 128 x 128 only, 3 / 4 / 5 / 6 / 7 force a form
    int s64;            // g_gemm_s64
    int small_x2;       // g_gemm_small_x2
    bool x3;            // bf16x3 build: operand images over K' = 3 K
    int ncu;
};
// What the planner needs to know about an epilogue functor (filled from the functor type by the launcher template).
struct EpiTraits {
    bool row_strip;     // lm_head partials: 64-column wave strips, no 192-wide tile
    bool strip_aux;
    bool dact;          // activation-gradient epilogue
    bool is_f32;        // EpiF32: the slab-writing functor, the only one that may be K-sliced over blockIdx.z on the 256-row kernels
    bool acc_init;      // can start its accumulators from its input (the kernels decide per form)
    bool x3;
};

// ---- which functor a wrapper runs ------------------------------------------------------------------------------------------------
enum EpiPick { EPI_GENERAL = 0, EPI_PLAIN, EPI_SPEC };
// gemm_bf16out: plain launches (no activation, no pre-activation copy, no operand image) take the functor without run-time switches; the
// c_fc forward of the training step (gelu_new, gelu' stored beside) its specialisation
inline EpiPick pick_bf16out(int act, bool pre, int img, const GemmKnobs& kn) {
    if (kn.epi_plain && act == 0 && !pre && img == 0) return EPI_PLAIN;
    if (kn.epi_spec && act == 3 && pre && !kn.pre_nt && img == 0) return EPI_SPEC;
    return EPI_GENERAL;
}
// gemm_dact: the forward stored gelu' (act 3): one multiply, no switch per unit
inline EpiPick pick_dact(int act, int img, const GemmKnobs& kn) { return (kn.epi_spec && act == 3 && img == 0) ? EPI_SPEC : EPI_GENERAL; }
// gemm_resid: accumulators initialised from the residual (256-row kernels only read the flag): not with residual dropout, whose mask scales
// acc + bias but not the residual
inline bool pick_resid_init(bool dropout, const GemmKnobs& kn) { return kn.resid_init && !dropout; }

// ---- NT launches (launch_gemm) -----------------------------------------------------------------------------------------------------
enum NtForm {
    NT_NOTHING = 0,     // empty problem or refusal: no launch
    NT_SKINNY,          // handed to the skinny launcher, form = skinny_form (the g_gemm_s64 > 0 hook)
    NT_STAG_256,        // gemm_nt_stag256_kernel<Epi, 4, false, 8>: 256 x 256
    NT_STAG_160,        //                       <Epi, 4, false, 5>: 160 x 256
    NT_STAG_320,        //                       <Epi, 4, false, 10>: 320 x 256
    NT_STAG_192,        //                       <Epi, 3, false, 8>: 256 x 192
    NT_STAG_192_X3F,    //                       <Epi, 3, false, 8, true>: its fused two-stage form (bf16x3)
    NT_Q4_3, NT_Q4_2,   // gemm_nt_q4_kernel<Epi, 5, 3 / 2>: persistent 160 x 256, three / two stages
    NT_ABLATION,        // gemm_nt_glds_kernel<Epi, abl>
    NT_GLDS4X2_X3F, NT_GLDS4X2, NT_GLDS4,      // small grids: 4-stage 128 x 128 forms
    NT_GLDS_X3F, NT_GLDS,                       // 128 x 128, two blocks per CU
    NT_REG_00, NT_REG_01, NT_REG_11             // gemm_bf16_kernel<al, bl>: register-staged, any layout
};
struct NtPlan {
    int status = CC_OK;
    NtForm form = NT_NOTHING;
    unsigned grid_x = 0, grid_z = 1, block = 0;
    size_t lds = 0;
    int k_chunk = 0, group_m = 8, stagger = 0, flags = 0;      // GemmShape fields
    int ks_eff = 1;
    int skinny_form = 0;      // NT_SKINNY
    int abl = 0;              // NT_ABLATION
};
// tile: -2 = process-wide mode / chooser, else as cc_gemm_tile_mode; group_m: row tiles per ordering group (0 = default)
inline NtPlan plan_nt(int al, int bl, int M, int N, int K, int lda, int ldb, int ksplit, int tile, int group_m, bool a_aligned, bool b_aligned,
                      const EpiTraits& t, const GemmModes& m, const GemmKnobs& kn) {
    NtPlan p;
    auto refuse = [&](int status) { p.status = status; return p; };
    if (M <= 0 || N <= 0 || K <= 0) return p;
    if ((lda & 7) || (ldb & 7) || !a_aligned || !b_aligned) return refuse(CC_ERR_SHAPE);
    if (al == 0 && (K & 7)) return refuse(CC_ERR_SHAPE);
    if (bl == 0 && (K & 7)) return refuse(CC_ERR_SHAPE);
    if (al == 1 && (M & 7)) return refuse(CC_ERR_SHAPE);
    if (bl == 1 && (N & 7)) return refuse(CC_ERR_SHAPE);
    const bool nt = al == 0 && bl == 0;
    if (!t.row_strip && !t.strip_aux && m.s64 > 0 && nt && (K % G_BK) == 0 && M <= 1024) {     // tools/small_gemm_bench.py (CC_GEMM_S64 = 1 / 2)
        p.form = NT_SKINNY;
        p.skinny_form = m.s64;
        return p;
    }
    p.group_m = kn.group_m > 0 ? kn.group_m : (group_m > 0 ? group_m : 8);
    p.stagger = kn.stagger;
    const KSlices sl = k_slices(K, G_BK, ksplit);
    ksplit = p.ks_eff = sl.ks_eff;
    p.k_chunk = sl.k_chunk;
    p.grid_z = (unsigned)ksplit;
    const long t128 = (long)((M + G_BM - 1) / G_BM) * ((N + G_BN - 1) / G_BN);
    // Tile choice for NT launches.  The 256-row kernel moves 1/2 (256 wide) or 2/3 (192 wide) of the 128 x 128 kernel's L2->LDS
    // bytes per flop and runs ~1.2x / ~1.15x its rate on full waves, but holds one block per CU, so wave quantisation decides:
    // cost = rounds x tile area / rate, the 128 x 128 kernel counted with 2 co-resident blocks per CU (measured table: DESIGN.md 4.1).
    // The 320 x 256 form (10 row tiles per wave, 36-KiB stages) does 1.25x the MFMAs per K-step at 1.13-1.27x the step time: it wins
    // where it saves a round (12800 x 3072: 480 tiles = 2 rounds instead of 3; the lm_head: 25 instead of 31).
    // g_gemm_tile_mode (cc_gemm_tile_mode / CC_GEMM_S256) = 0 (never) / 3 / 4 / 5 / 6 (force 256x192 / 256x256 / 320x256 / 160x256) overrides it for
    // tests and tools/gemm_tiles.py.
    const int s256 = tile != -2 ? tile : m.tile_mode;
    int nj = 0, ni = 8;
    const bool can160 = !t.x3 && !t.row_strip && !t.dact;      // the 160 x 256 form (below)
    // K slices (blockIdx.z) on the 256-row kernels only for the slab-writing fp32 epilogue and only when the caller names the tile
    const bool zsplit_ok = t.is_f32;
    if (nt && (K % H_BK) == 0 && (ksplit == 1 || (zsplit_ok && tile > 0)) && s256 != 0) {
        const long tm = (M + H_BM - 1) / H_BM;
        const long t256 = tm * ((N + 255) / 256), t192 = tm * ((N + 191) / 192), t320 = (long)((M + 319) / 320) * ((N + 255) / 256);
        const double c128 = t128 <= 256 ? 16384.0 / 0.75 : (double)((t128 + 511) / 512) * 32768.0;
        // (bf16x3 build, round 5: crediting the 256 x 192 form with its fused two-stage loop — c192 / 1.45, which moves c_attn / c_fc forward from
        // the three-pass 256-wide forms to 3-4 rounds of fused 192-wide tiles — measured 28.55 -> 30.1 ms per step, two alternations: reverted)
        const double c256 = (double)((t256 + 255) / 256) * 65536.0 / 1.2, c192 = (double)((t192 + 255) / 256) * 49152.0 / 1.15;
        const double c320 = (double)((t320 + 255) / 256) * 81920.0 / 1.3;
        const bool can192 = !t.row_strip;   // the lm_head partials assume 64-column wave strips
        // the activation-gradient epilogue (aux tile read + gelu' + store) is not hidden at one block per CU: 12800 x 3072 x 768 measured
        // 106.6 us on 320 x 256 vs 97.3 on 128 x 128 (two co-resident blocks), while the plain / gelu-forward epilogues gain (90 -> 78 us)
        // (also with the forward-stored derivative, act 3 — a single multiply —, the 128 x 128 kernel stays ahead: 12.31 vs 12.44 ms per step)
        const bool can320 = !t.dact;
        // (round 5) 160 x 256 (5 row tiles per wave, 26-KiB stages): for the N = 768 launches at M = 12800 it is 240 tiles on the 256 CUs where
        // 256 x 192 is 200 — hipBLASLt's pick for these shapes too (MT160x256, profiles/r05_j_*).  A single-round launch takes one tile's
        // latency, so the smaller tile is the shorter launch whenever both fit one round; never for the bf16x3 build (its fused form is 192-wide).
        const long t160 = (long)((M + 159) / 160) * ((N + 255) / 256);
        const double c160 = (double)((t160 + 255) / 256) * 40960.0 / 1.1;
        if (can160 && (s256 == 6 || s256 == 7 || (s256 < 0 && kn.s160 && ksplit == 1 && c160 < 0.98 * c128 && c160 < 0.98 * c256 && c160 < 0.98 * c320 && (!can192 || c160 < 0.98 * c192)))) { nj = 4; ni = 5; }
        else if (s256 == 5 || (can320 && s256 < 0 && c320 < 0.98 * c128 && c320 < c256 && (!can192 || c320 < c192))) { nj = 4; ni = 10; }
        else if (s256 == 4 || (s256 < 0 && c256 < 0.98 * c128 && (!can192 || c256 <= c192))) nj = 4;
        else if (can192 && (s256 == 3 || (s256 < 0 && c192 < 0.98 * c128))) nj = 3;
    }
    const bool x3f = t.x3 && kn.x3_fused;      // bf16x3 build: the fused two-stage forms of the NT kernels
    if (nj) {
        const int bm = 32 * ni;
        p.block = 512;
        p.lds = (size_t)H_NS * (bm + H_BN) * H_BK * 2;
        p.grid_x = (unsigned)(((M + bm - 1) / bm) * ((N + 64 * nj - 1) / (64 * nj)));
        if (nj == 4 && ni == 8) p.form = NT_STAG_256;
        else if (nj == 4 && ni == 5) {
            // (round 6) the 160 x 256 launches go to the persistent 4-wave kernel with 64-deep full-line stages (gemm_q4.hip.h) wherever K fits its
            // ring: three stages for K % 192 == 0, two for K % 128 == 0; byte offsets inside an operand are 32-bit there.  Measured against the
            // staggered 160 x 256 kernel (profiles/r06_l): 12800 x 768 x 3072 58.9 -> 52.8 us, x 2304 44.2 -> 41.7, x 768 20.2 -> 21.2 (plain functor:
            // 57.1 -> 49.7, 43.7 -> 38.5, 20.6 -> 19.8).  cc_gemm_tile_mode 6 keeps the staggered kernel, 7 forces this one.
            const bool fits32 = (size_t)M * (size_t)lda * 2 < 0xffff0000ull && (size_t)N * (size_t)ldb * 2 < 0xffff0000ull;
            const int ns = (K % 192 == 0 && K >= 384) ? 3 : ((K % 128 == 0 && K >= 256) ? 2 : 0);
            p.flags = kn.q4_last ? 0 : 1;
            p.form = NT_STAG_160;
            if (ns && fits32 && ksplit == 1 && s256 != 6 && (kn.q4 || s256 == 7)) {
                const int tiles = ((M + 159) / 160) * ((N + 255) / 256);
                p.form = ns == 3 ? NT_Q4_3 : NT_Q4_2;
                p.grid_x = (unsigned)(tiles < m.ncu ? tiles : m.ncu);
                p.grid_z = 1;
                p.block = 256;
                p.lds = (size_t)ns * (160 + 256) * 128;
            }
        }
        else if (nj == 4) p.form = NT_STAG_320;
        else      // bf16x3 build: every NT launch carries operand images over K' = 3 K — the fused two-stage form (gemm_stag256_body, X3F)
            p.form = (x3f && (K % (3 * H_BK)) == 0 && ksplit <= K / (3 * H_BK)) ? NT_STAG_192_X3F : NT_STAG_192;     // (K slices: ranges of the logical K's chunks, every slice non-empty)
        return p;
    }
    p.grid_x = (unsigned)t128;
    p.block = G_THREADS;
    const bool dma = nt && (K % G_BK) == 0;
    if (dma && (kn.abl == 1 || kn.abl == 2 || kn.abl == 4 || kn.abl == 5 || kn.abl == 6)) {
        p.form = NT_ABLATION;
        p.abl = kn.abl;
    } else if (dma && t128 * ksplit <= 256 && m.tile_mode != 0 && K / ksplit >= 4 * G_BK) {
        // at most one block per CU: nothing co-resident to hide the 2-stage kernel's per-K-step round trip -> 4-stage variant
        p.lds = (size_t)8 * G_TILE_BYTES;
        if (m.small_x2 && x3f && ksplit == 1 && (K % (3 * G_BK)) == 0) p.form = NT_GLDS4X2_X3F;
        else p.form = m.small_x2 ? NT_GLDS4X2 : NT_GLDS4;
        if (m.small_x2) p.block = 2 * G_THREADS;
    } else if (dma) {
        // bf16x3 build: operand images over K' = 3 K -> the fused two-stage form
        p.form = (x3f && ksplit == 1 && (K % (3 * G_BK)) == 0) ? NT_GLDS_X3F : NT_GLDS;
    }
    else if (al == 0 && bl == 0) p.form = NT_REG_00;
    else if (al == 0 && bl == 1) p.form = NT_REG_01;
    else if (al == 1 && bl == 1) p.form = NT_REG_11;
    else return refuse(CC_ERR_ARG);
    return p;
}

// ---- skinny NT launches (launch_gemm_s64): K % 64 == 0, K slices over blockIdx.z ----------------------------------------------------
// form 1 (64 x 64 tiles), 2 (64 x 128), 3 (64 x 64, K over the waves), 4 (80 x 64, K over the waves); lab build: form 3 with the weight
// operand global -> VGPR from its fragment-ordered image (S64_IMAGE)
constexpr int S64_IMAGE = 5;
struct S64Plan {
    int status = CC_OK;
    int form = 1;
    unsigned grid_x = 0, grid_z = 1, block = G_THREADS;
    size_t lds = 0;
    int k_chunk = 0, ks_eff = 1;
};
inline S64Plan plan_s64(int M, int N, int K, int lda, int ldb, int ksplit, int nj, bool a_aligned, bool b_aligned, bool image_usable) {
    S64Plan p;
    if ((K % G_BK) || (lda & 7) || (ldb & 7) || !a_aligned || !b_aligned) { p.status = CC_ERR_SHAPE; return p; }
    const KSlices sl = k_slices(K, G_BK, ksplit);
    p.ks_eff = sl.ks_eff;
    p.k_chunk = sl.k_chunk;
    p.grid_z = (unsigned)sl.ks_eff;
    const int tm = (M + 63) / 64;
#ifdef CC_EXPERIMENTS
    if (nj == 3 && image_usable && (N % 64) == 0) {
        p.form = S64_IMAGE;
        p.lds = (size_t)4 * 128 * 128;      // (the epilogue's partial tiles need the 64 KiB)
        p.grid_x = (unsigned)(tm * (N / 64));
        p.block = 320;
        return p;
    }
#else
    (void)image_usable;
#endif
    if (nj == 4) {                   // 80 x 64 tiles, K split over the waves (gemm_nt_s80kw_kernel)
        p.form = 4;
        p.lds = (size_t)4 * 6 * 16 * 64 * sizeof(float);      // the epilogue's partial tiles: 96 KiB (the four 20-KiB stages fit inside)
        p.grid_x = (unsigned)(((M + 79) / 80) * ((N + 63) / 64));
    } else if (nj == 3) {            // K split over the waves (gemm_nt_s64kw_kernel)
        p.form = 3;
        p.lds = (size_t)4 * 128 * 128;
        p.grid_x = (unsigned)(tm * ((N + 63) / 64));
    } else if (nj == 2) {
        p.form = 2;
        p.lds = (size_t)3 * (64 + 128) * 128;
        p.grid_x = (unsigned)(tm * ((N + 127) / 128));
    } else {
        p.form = 1;
        p.lds = (size_t)4 * (64 + 64) * 128;
        p.grid_x = (unsigned)(tm * ((N + 63) / 64));
    }
    return p;
}

// ---- gemm_nt_skinny: single pass or K-sliced slabs + one finishing kernel ------------------------------------------------------------
enum SkinnyFunctor { SK_RESID, SK_PLAIN, SK_GELU, SK_BF16, SK_F32 };      // single pass: EpiResid, EpiBF16Plain, EpiBF16T<2, 0>, EpiBF16, EpiF32
enum SkinnyFinish { FIN_ROW, FIN_FLAT, FIN_REFUSE };                       // k_splitk_finish_row, k_splitk_finish, or CC_ERR_SHAPE after the slab launch
struct SkinnyPlan {
    int status = CC_OK;
    bool s64 = false;         // on the 64-row kernels (form below), else through launch_gemm
    bool slab = false;        // K slices into fp32 slabs + finish, else single pass with the epilogue fused
    int ks = 1;               // requested slices
    int form = 0;
    SkinnyFunctor functor = SK_F32;
    SkinnyFinish finish = FIN_ROW;
};
// M, N, K, lda, ldb as the kernel reads them (bf16x3: the image's); fused = a SkinnyFuse tail was requested
inline SkinnyPlan plan_skinny(int M, int N, int K, int lda, int ldb, bool has_scratch, size_t scratch_bytes, bool fused, bool has_res, bool has_out16,
                              int act, const GemmModes& m, const GemmKnobs& kn) {
    SkinnyPlan p;
    const int tiles = ((M + G_BM - 1) / G_BM) * ((N + G_BN - 1) / G_BN);
    const size_t slab = (size_t)M * N;
    const bool can_slab = has_scratch && slab && (K % G_BK) == 0 && scratch_bytes >= slab * sizeof(float);
    // decode-sized M: 64 x 64 tiles (gemm_nt_s64_kernel) put 2.5-5x the blocks on the chip; a block's K loop is bound by what one CU
    // can pull through its L2->LDS path (~57 GB/s measured), so the job is to have every CU pulling
    p.s64 = m.s64 != 0 && (K % G_BK) == 0 && M <= 640 && tiles <= 256 && (lda & 7) == 0 && (ldb & 7) == 0;
    int ks;
    if (p.s64) {
        const int t64 = ((M + 63) / 64) * ((N + 63) / 64);
        ks = t64 >= 160 ? 1 : 256 / t64;                    // K slices only while they add blocks up to one per CU
        const int kmax = K / (4 * G_BK);
        if (ks > kmax) ks = kmax;
    } else {
        ks = 384 / (tiles > 0 ? tiles : 1);
        const int kmax = K / (2 * G_BK);                    // at least 2 K-steps per slice
        if (ks > kmax) ks = kmax;
        // wide-enough grids go single-pass with the epilogue fused into the GEMM (4-stage small-grid kernel): one launch instead of two
        if (!fused && tiles >= kn.skinny_single) ks = 1;
    }
    if (ks < 1) ks = 1;
    if (can_slab) { const size_t fit = scratch_bytes / (slab * sizeof(float)); if ((size_t)ks > fit) ks = (int)fit; }
    // K split over the waves of a block (gemm_nt_s64kw_kernel): pays from ~14 K-tiles per block, and only on grids of at most one
    // block per CU (320 x 3072 x 1024: 9.0 -> 8.3 us, 320 x 1024 x 4096 in one slice: 23.6 -> 18.4 us; c_fc's 320 blocks: no gain)
    // (round 5) a single-slice grid of 257-320 64 x 64 tiles that is <= 256 tiles of 80 x 64 (c_fc at M = 320: 5 x 64 -> 4 x 64) takes the
    // 80-row form of the same kernel: one block per CU instead of two on a quarter of them (CC_SKINNY_80=0 in the lab build: off)
    auto s64_form = [&](int slices) {
        const int t64 = ((M + 63) / 64) * ((N + 63) / 64), t80 = ((M + 79) / 80) * ((N + 63) / 64);
        if (m.s64 == 1 || K / G_BK / (slices > 0 ? slices : 1) < 14) return 1;
        if ((long)t64 * slices <= 256) return 3;
        return (kn.skinny_80 && slices <= 1 && t80 <= 256) ? 4 : 1;      // (no weight-image variant: both operand paths run this kernel)
    };
    if (!can_slab || (ks <= 1 && !fused)) {
        if (fused) { p.status = CC_ERR_SHAPE; return p; }      // callers only request fusion when the slab path is available
        p.ks = 1;
        p.form = p.s64 ? s64_form(1) : 0;
        if (has_res) p.functor = SK_RESID;
        else if (has_out16) {
            // decode's c_attn (plain) and c_fc (gelu_new) launches on the 64-row kernels: the functors without run-time switches (round 6)
            p.functor = (p.s64 && kn.epi_spec && act == 0) ? SK_PLAIN : (p.s64 && kn.epi_spec && act == 2) ? SK_GELU : SK_BF16;
        } else p.functor = SK_F32;
        return p;
    }
    p.slab = true;
    p.ks = ks;
    p.form = p.s64 ? s64_form(ks) : 0;
    p.finish = (N <= 3072 && (N & 3) == 0) ? FIN_ROW : (fused ? FIN_REFUSE : FIN_FLAT);
    return p;
}

// ---- gemm_nt_deepk: narrow output, very deep K, on whole rounds of K slices --------------------------------------------------------
struct DeepKPlan {
    int status = CC_OK;         // refusal before the operand is prepared
    int status_late = CC_OK;    // refusal after it (bf16x3 search)
    int ks = 0, tile = 4, group_m = 1;
};
// M, N, K, lda, ldb: the caller's logical values (bf16x3: the planner reads K' = 3 K where the kernel does)
inline DeepKPlan plan_deepk(int M, int N, int K, int lda, int ldb, int ldo, bool has_scratch, size_t scratch_bytes, const GemmModes& m, const GemmKnobs& kn) {
    DeepKPlan p;
    if (kn.deepk == 0 || m.tile_mode == 0 || !has_scratch || (N & 7) || (ldo & 7) || (K % 64) || (lda & 7) || (ldb & 7)) { p.status = CC_ERR_SHAPE; return p; }
    const long tiles = (long)((M + H_BM - 1) / H_BM) * ((N + H_BN - 1) / H_BN);
    const size_t slab = (size_t)M * N;
    int ks = kn.deepk > 0 ? kn.deepk : (int)(256 / (tiles > 0 ? tiles : 1));
    const size_t fit = scratch_bytes / (slab * sizeof(float));
    if ((size_t)ks > fit) ks = (int)fit;
    if (ks > K / 2048) ks = K / 2048;                      // slices of at least 64 K-steps: below that the slab pass costs what the idle CUs gain
    if (ks < 2 || tiles > 128) { p.status = CC_ERR_SHAPE; return p; }
    // tile order: an XCD's share of the grid (tiles / 8 consecutive logical tiles per K slice) should hold whole row panels, so that the
    // column tiles of a panel run side by side on one L2 and the deep A panel is fetched once, not once per column tile
    int tiles_n = (N + H_BN - 1) / H_BN;
    long tl = tiles;
    const int K3 = 3 * K;
    if (m.x3 && kn.x3_fused && (K3 % (3 * H_BK)) == 0) {
        // bf16x3: the fused two-stage form lives on the 256 x 192 kernel (gemm_stag256_body<X3F>): its tile count, and the slice count
        // that minimises rounds x chunks per slice (whole rounds of 256 workgroups)
        p.tile = 3;
        tiles_n = (N + 191) / 192;
        tl = (long)((M + H_BM - 1) / H_BM) * tiles_n;
        const int nc = K3 / (3 * H_BK);
        long best = -1;
        int best_ks = ks;
        for (int k2 = 1; k2 <= 8 && (size_t)k2 <= fit && k2 <= nc / 32; k2++) {
            const long cost = ((tl * k2 + 255) / 256) * ((nc + k2 - 1) / k2);
            if (best < 0 || cost < best) { best = cost; best_ks = k2; }
        }
        ks = best_ks;
        if (ks < 2) p.status_late = CC_ERR_SHAPE;
    }
    p.ks = ks;
    p.group_m = (int)((tl + 7) / 8) / tiles_n;
    if (p.group_m < 1) p.group_m = 1;
    return p;
}

// ---- weight-gradient (TT) launchers: launch_gemm_tt256 / tt128, K slices over blockIdx.z ---------------------------------------------
struct TTPlan {
    int status = CC_OK;
    unsigned grid_x = 0, grid_z = 1, block = 0;
    size_t lds = 0;
    int k_chunk = 0, ks_eff = 1;
};
// tile 256: the 256 x 256 kernel with direct-to-LDS staging and transpose reads (K % 32 == 0); tile 128: gemm_tt_glds4_kernel (K % 64 == 0)
inline TTPlan plan_tt(int tile, int M, int N, int K, int lda, int ldb, int ksplit, bool a_aligned, bool b_aligned) {
    TTPlan p;
    const int bk = tile == 256 ? H_BK : G_BK;
    if ((K % bk) || (M & 7) || (N & 7) || (lda & 7) || (ldb & 7) || !a_aligned || !b_aligned) { p.status = CC_ERR_SHAPE; return p; }
    const KSlices sl = k_slices(K, G_BK, ksplit);
    p.ks_eff = sl.ks_eff;
    p.k_chunk = sl.k_chunk;
    p.grid_x = (unsigned)(((M + tile - 1) / tile) * ((N + tile - 1) / tile));
    p.grid_z = (unsigned)sl.ks_eff;
    p.block = tile == 256 ? 512 : G_THREADS;
    p.lds = tile == 256 ? (size_t)H_NS * H_STAGE : (size_t)8 * G_TILE_BYTES;
    return p;
}

// ---- gemm_wgrad: one weight gradient on its own -----------------------------------------------------------------------------------
enum WgradForm {
    WG_TT256_DIRECT,    // 256 x 256, one slice, dW += tile in the epilogue
    WG_TT256_SLABS,     // 256 x 256, K slices into slabs + reduce
    WG_TT128_SLABS,     // 128 x 128 TT kernel, K slices into slabs + reduce
    WG_REG_DIRECT,      // register-staged kernel (any alignment), dW += tile
    WG_REG_SLABS        // register-staged kernel, K slices into slabs + reduce
};
struct WgradPlan { WgradForm form; int ks; };
// tt_ok: operands and row strides 16-B aligned; room: bytes of scratch behind the batch's parked slabs (ignored without scratch)
inline WgradPlan plan_wgrad(int Mw, int Nw, int K, bool tt_ok, bool has_scratch, size_t room, const GemmModes& m) {
    const size_t slab = (size_t)Mw * Nw;
    const size_t fit = has_scratch ? room / (slab * sizeof(float)) : 1;
    // 256 x 256 kernel with DMA staging + transpose reads (one block per CU; slices sized to fill the CUs once).  It wins from
    // about 30 GFLOP per launch (GPT-2 weight gradients: +10...17 %); below that the 128 x 128 TT kernel's finer tiles and fewer,
    // smaller slabs win (mapper weight gradients, K = 5120) — tools/wgrad_bench.py.
    if (m.tile_mode != 0 && tt_ok && (K % H_BK) == 0 && (m.tile_mode == 4 || 2.0 * Mw * Nw * (double)K >= 3e10)) {
        const int tiles = ((Mw + H_BM - 1) / H_BM) * ((Nw + H_BN - 1) / H_BN);
        int ks = 256 / tiles > 1 ? 256 / tiles : 1;
        const int kmax = K / 512 > 1 ? K / 512 : 1;       // at least 16 K-tiles per slice
        if (ks > kmax) ks = kmax;
        if ((size_t)ks > fit) ks = (int)(fit > 1 ? fit : 1);
        return {ks == 1 ? WG_TT256_DIRECT : WG_TT256_SLABS, ks};      // (one slice: wide outputs (lm_head) accumulate straight into dW)
    }
    const int tiles = ((Mw + G_BM - 1) / G_BM) * ((Nw + G_BN - 1) / G_BN);
    // small weight gradients (mapper, K = 5120): 128 x 128 TT kernel, 4-stage DMA pipeline + transpose reads, one block per CU
    if (m.tile_mode != 0 && tt_ok && (K % G_BK) == 0 && K >= 1024 && tiles <= 256 && has_scratch && fit >= 1) {
        int ks = 256 / tiles > 1 ? 256 / tiles : 1;
        const int kmax = K / (4 * G_BK) > 1 ? K / (4 * G_BK) : 1;
        if (ks > kmax) ks = kmax;
        if ((size_t)ks > fit) ks = (int)fit;
        return {WG_TT128_SLABS, ks};
    }
    int ks = 512 / (tiles > 0 ? tiles : 1);
    const int kmax = (K + 255) / 256;  // at least 4 K-steps per slice
    if (ks > kmax) ks = kmax;
    if (has_scratch) { if ((size_t)ks > fit) ks = (int)fit; } else ks = 1;
    return {ks <= 1 ? WG_REG_DIRECT : WG_REG_SLABS, ks};
}

// ---- wgrad_launch_group: the deferred problems of a batch (same K) as one grouped launch ------------------------------------------------
constexpr int TT_GROUP_MAX = 32;
struct WgradProblem { int Mw, Nw; };
struct WgradGroupPlan {
    int status = CC_OK;
    int tile = 128;                     // 256: gemm_tt_stag256_group_kernel, 128: gemm_tt_glds4_group_kernel
    int ks = 1, k_chunk = 0;            // slices per problem and their depth
    int first[TT_GROUP_MAX + 1];        // logical block ranges of the problems
    int whole = -1, split = 1;          // direct form: K-sliced tail (TTGroup::whole / split)
    unsigned blocks = 0, block = 0, reduce_blocks = 0;      // grid and block of the launch; grid of gemm_tt_tail_reduce_kernel (0: none)
    size_t lds = 0;
};
inline void plan_group_launch(WgradGroupPlan& p, int nd) {
    for (int i = nd + 1; i <= TT_GROUP_MAX; i++) p.first[i] = p.first[nd];
    const int total = p.first[nd];
    p.blocks = p.whole >= 0 ? (unsigned)(p.whole + (total - p.whole) * p.split) : (unsigned)total;
    p.reduce_blocks = p.whole >= 0 ? (unsigned)(total - p.whole) * 16 : 0;
    p.block = p.tile == 256 ? 512 : G_THREADS;
    p.lds = p.tile == 256 ? (size_t)H_NS * H_STAGE : (size_t)4 * 2 * G_TILE_BYTES;
}
// direct form: one K slice per tile, dW += tile in the epilogue: the 256 x 256 kernel when K allows it (a block walks the whole K: 160 steps
// at K = 5120).  tail_ok: the batch has scratch that nothing else uses; tail_room: its bytes
inline WgradGroupPlan plan_wgrad_group_direct(const WgradProblem* d, int nd, int K, bool tail_ok, size_t tail_room, const GemmKnobs& kn) {
    WgradGroupPlan p;
    const bool t256 = (K % H_BK) == 0;
    p.tile = t256 ? 256 : 128;
    p.k_chunk = k_slices(K, G_BK, 1).k_chunk;
    int first = 0;
    for (int i = 0; i < nd; i++) {
        p.first[i] = first;
        first += ((d[i].Mw + p.tile - 1) / p.tile) * ((d[i].Nw + p.tile - 1) / p.tile);
    }
    p.first[nd] = first;
    if (t256) {
        // the tail beyond the last full round of 256 workgroups: K slices + a small reduce, so that it is a short round of every CU
        // (CC_WGRAD_TAIL=0 in the lab build: whole tiles only)
        const int full = (first / 256) * 256, rem = first - full;
        int sp = rem > 0 ? 256 / rem : 1;
        int cap = (K / H_BK) / 16;      // at least 16 K-steps per slice
        cap = cap < 1 ? 1 : (cap > 8 ? 8 : cap);
        if (sp > cap) sp = cap;
        // (the slices' slabs: rem x sp x 256 KiB <= 64 MiB of the scratch, which a direct batch does not use otherwise)
        if (kn.wgrad_tail && full > 0 && sp >= 2 && tail_ok && (size_t)rem * sp * H_BM * H_BN * sizeof(float) <= tail_room) {
            p.whole = full;
            p.split = sp;
        }
    }
    plan_group_launch(p, nd);
    return p;
}
// slab form: a common slice count ks is chosen to minimise rounds x (K-steps per block + fixed per-block cost), rounds = ceil(blocks / CUs);
// tile kernel: 256 x 256 (8 waves, fewer / fatter blocks) or 128 x 128.  CC_WGRAD_TILE / CC_WGRAD_KS override (tuning knobs).
// room: bytes of scratch behind the parked slabs
inline WgradGroupPlan plan_wgrad_group(const WgradProblem* d, int nd, int K, size_t room, const GemmKnobs& kn) {
    WgradGroupPlan p;
    size_t slab_sum = 0;
    for (int i = 0; i < nd; i++) slab_sum += (((size_t)d[i].Mw * d[i].Nw * sizeof(float)) + 255) & ~size_t(255);
    int best_tile = 128, best_ks = 1;
    double best_cost = 1e30;
    for (int tile : {256, 128}) {
        if (kn.wgrad_tile && tile != kn.wgrad_tile) continue;
        if (tile == 256 && (K % H_BK)) continue;
        const int bk = tile == 256 ? H_BK : G_BK, ksteps = K / bk;
        int total = 0;
        for (int i = 0; i < nd; i++) total += ((d[i].Mw + tile - 1) / tile) * ((d[i].Nw + tile - 1) / tile);
        // per K-step cost in units of a 128-tile step (measured: 256-tile step of 32 ~ 0.8 us for 4x the tile area, 128-tile step of 64 ~ 0.65 us)
        const double step_cost = tile == 256 ? 1.25 : 1.0, fixed = tile == 256 ? 16.0 : 14.0;
        for (int ks = 1; ks <= 8 && (size_t)ks * slab_sum <= room && ksteps / ks >= 8; ks++) {
            if (kn.wgrad_ks && ks != kn.wgrad_ks) continue;
            const int per = (ksteps + ks - 1) / ks;
            const int rounds = (total * ks + 255) / 256;
            const double cost = rounds * (per * step_cost + fixed);
            if (cost < best_cost) { best_cost = cost; best_tile = tile; best_ks = ks; }
        }
    }
    if (best_cost >= 1e30) { p.status = CC_ERR_STATE; return p; }      // no (tile, slices) fits the scratch: gemm_wgrad's admission check keeps this from happening
    // slices are multiples of 64 deep for both kernels (k_chunk convention of GemmShape)
    const KSlices sl = k_slices(K, G_BK, best_ks);
    p.tile = best_tile;
    p.ks = sl.ks_eff;
    p.k_chunk = sl.k_chunk;
    int first = 0;
    for (int i = 0; i < nd; i++) {
        p.first[i] = first;
        first += ((d[i].Mw + best_tile - 1) / best_tile) * ((d[i].Nw + best_tile - 1) / best_tile) * p.ks;
    }
    p.first[nd] = first;
    plan_group_launch(p, nd);
    return p;
}

}  // namespace cc_plan
