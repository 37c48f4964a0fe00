// Stand-alone check of the launch plans the MLP mapping network's backward gets from clipcap_amd/csrc/gemm_plan.h at its real shape
// (E = 512, D = 768, L = 10: model.2.weight is 7680 x 3840), compiled by tests/test_mlp_surface.py with the host compiler alone.
// One fp32 slab of model.2.weight is 118 MB, more than the 96 MiB of weight-gradient scratch (gemm_api.h WGRAD_SCRATCH_BYTES): no slab form
// can be planned, whatever the batch — the gradient must come out of a one-slice form that adds into dW in its epilogue.
#include <cstdio>
#include "gemm_plan.h"

using namespace cc_plan;
static int failures = 0;
#define CHECK(cond, ...)                                                                 \
    do {                                                                                 \
        if (!(cond)) { failures++; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

int main() {
    const size_t scratch = size_t(96) << 20;      // WGRAD_SCRATCH_BYTES of the product
    const int Hd = 3840, LD = 7680, E = 512;
    CHECK((size_t)Hd * LD * sizeof(float) > scratch, "one slab of model.2.weight fits the scratch after all");
    long checked = 0;
    for (bool x3 : {false, true}) {
        const GemmModes m{-1, -1, 1, x3, 256};
        for (int B : {16, 256, 1024, 4096}) {
            const int K = x3 ? 3 * B : B;
            for (bool swap : {false, true}) {      // dW2 = g16^T h is (L D) x Hd; the transposed problem plans the same way
                const WgradPlan p = plan_wgrad(swap ? LD : Hd, swap ? Hd : LD, K, true, true, scratch, m);
                CHECK(p.ks <= 1, "B %d x3 %d: %d slices of a slab that does not fit", B, (int)x3, p.ks);
                CHECK(p.form == WG_REG_DIRECT || p.form == WG_TT256_DIRECT, "B %d x3 %d: form %d is not a direct form", B, (int)x3, (int)p.form);
                checked += 2;
            }
        }
        // the issue's case: B = 256, bf16 operands -> below the 256 x 256 kernel's 30 GFLOP threshold, 1800 tiles of 128 x 128: the register-staged direct form
        if (!x3) {
            const WgradPlan p = plan_wgrad(Hd, LD, 256, true, true, scratch, m);
            CHECK(p.form == WG_REG_DIRECT && p.ks <= 1, "form %d ks %d", (int)p.form, p.ks);
            const WgradPlan q = plan_wgrad(Hd, LD, 1024, true, true, scratch, m);
            CHECK(q.form == WG_TT256_DIRECT && q.ks == 1, "B = 1024: form %d ks %d", (int)q.form, q.ks);
            checked += 2;
        }
        // dW1 = dU^T x16 is Hd x E: 7.9 MB a slab, so it may be sliced, but never into more slabs than fit
        for (int B : {16, 256, 1024}) {
            const WgradPlan p = plan_wgrad(Hd, E, x3 ? 3 * B : B, true, true, scratch, m);
            CHECK(p.ks >= 0 && (size_t)(p.ks > 1 ? p.ks : 1) * Hd * E * sizeof(float) <= scratch, "dW1 B %d: %d slabs", B, p.ks);
            checked++;
        }
    }
    printf("%s: %ld checks, %d failures\n", failures ? "FAILED" : "ok", checked, failures);
    return failures ? 1 : 0;
}
