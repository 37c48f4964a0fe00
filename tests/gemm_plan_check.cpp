// Stand-alone check of clipcap_amd/csrc/gemm_plan.h (tests/test_gemm_plan.py compiles it with the host compiler alone — no HIP include
// path — and once more with -fsanitize=address,undefined): the K-slice function's invariants, and the rows of DESIGN.md 4.1's tile table
// that state a choice.
#include <cstdio>
#include <initializer_list>
#include "gemm_plan.h"

using namespace cc_plan;
static int failures = 0;
#define CHECK(cond, ...)                                                                 \
    do {                                                                                 \
        if (!(cond)) { failures++; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

int main() {
    // ---- K slices: non-empty, whole steps, cover K exactly once
    long checked = 0;
    for (int step : {32, 64})
        for (int K = 64; K <= 8192; K += 32)
            for (int want = 1; want <= 9; want++) {
                const KSlices s = k_slices(K, step, want);
                CHECK(s.ks_eff >= 1 && s.ks_eff <= want, "K %d step %d want %d: ks_eff %d", K, step, want, s.ks_eff);
                CHECK(s.k_chunk > 0 && s.k_chunk % step == 0, "K %d step %d want %d: k_chunk %d", K, step, want, s.k_chunk);
                CHECK((long)s.ks_eff * s.k_chunk >= K, "K %d step %d want %d: %d x %d does not cover K", K, step, want, s.ks_eff, s.k_chunk);
                CHECK((long)(s.ks_eff - 1) * s.k_chunk < K, "K %d step %d want %d: slice %d is empty", K, step, want, s.ks_eff - 1);
                checked++;
            }
    CHECK(k_slices(768, 64, 0).ks_eff == 1 && k_slices(768, 64, -3).k_chunk == 768, "fewer than one slice wanted");

    // ---- the product build's frozen switches, default modes, 256 CUs
    const GemmKnobs kn;
    const GemmModes bf16{-1, -1, 1, false, 256};
    const EpiTraits plain{false, false, false, false, false, false}, resid{false, false, false, false, true, false};
    auto nt = [&](int M, int N, int K, const EpiTraits& t, const GemmModes& m, int ksplit = 1, int tile = -2) {
        return plan_nt(0, 0, M, N, K, K, K, ksplit, tile, 0, true, true, t, m, kn);
    };
    {   // c_fc forward: 12800 x 3072 x 768 takes the 320 x 256 form in two rounds
        const NtPlan p = nt(12800, 3072, 768, plain, bf16);
        CHECK(p.status == CC_OK && p.form == NT_STAG_320, "form %d", (int)p.form);
        CHECK(p.grid_x == 480 && p.grid_z == 1 && p.block == 512 && (p.grid_x + 255) / 256 == 2, "grid %u", p.grid_x);
        CHECK(p.lds == (size_t)H_NS * (320 + 256) * H_BK * 2, "lds %zu", p.lds);
    }
    // the N = 768 launches at M = 12800: the persistent 160 x 256 kernel, three stages when K % 192 == 0, two when only K % 128 == 0
    for (const EpiTraits& t : {plain, resid})
        for (int K : {768, 2304, 3072, 1024}) {
            const NtPlan p = nt(12800, 768, K, t, bf16);
            CHECK(p.form == (K % 192 == 0 ? NT_Q4_3 : NT_Q4_2), "K %d: form %d", K, (int)p.form);
            CHECK(p.grid_x == 240 && p.grid_z == 1 && p.block == 256, "K %d: grid %u block %u", K, p.grid_x, p.block);
            CHECK(p.lds == (size_t)(K % 192 == 0 ? 3 : 2) * (160 + 256) * 128, "K %d: lds %zu", K, p.lds);
        }
    CHECK(nt(12800, 768, 768, plain, GemmModes{-1, -1, 1, false, 64}).grid_x == 64, "the persistent grid is capped at the CU count");
    // sweeps: the bf16x3 build never takes a 160-row form; row-strip epilogues never take a 192-wide tile — under every tile mode
    for (int mode : {-1, 0, 3, 4, 5, 6, 7})
        for (int M = 64; M <= 25600; M += M < 2048 ? 192 : 1280)
            for (int N : {192, 384, 768, 1024, 2304, 3072, 4096, 50304})
                for (int K : {96, 768, 1024, 3072}) {
                    EpiTraits tx = plain, strip = plain;
                    tx.x3 = true;
                    strip.row_strip = true;
                    const NtPlan a = nt(M, N, 3 * K, tx, GemmModes{mode, -1, 1, true, 256});
                    CHECK(a.form != NT_STAG_160 && a.form != NT_Q4_3 && a.form != NT_Q4_2, "bf16x3 %d x %d x %d mode %d: form %d", M, N, K, mode, (int)a.form);
                    const NtPlan b = nt(M, N, K, strip, GemmModes{mode, -1, 1, false, 256});
                    CHECK(b.form != NT_STAG_192 && b.form != NT_STAG_192_X3F && b.form != NT_STAG_160 && b.form != NT_Q4_3 && b.form != NT_Q4_2,
                          "row strip %d x %d x %d mode %d: form %d", M, N, K, mode, (int)b.form);
                    strip.x3 = true;
                    const NtPlan c = nt(M, N, 3 * K, strip, GemmModes{mode, -1, 1, true, 256});
                    CHECK(c.form != NT_STAG_192 && c.form != NT_STAG_192_X3F, "row strip, bf16x3 %d x %d x %d mode %d: form %d", M, N, K, mode, (int)c.form);
                    checked += 3;
                }
    printf("%s: %ld checks, %d failures\n", failures ? "FAILED" : "ok", checked, failures);
    return failures ? 1 : 0;
}
