#include "gemm.hip.h"
#include "gemm_api.h"
namespace CC_NS {
int gemm_bf16out(int al, int bl, ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, Act Co, int ldc,
                 const float* bias, int act, act_t* pre, Call& cx) {
    const hipStream_t st = cx.st;
    act_t* const C = Co.p;
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, 2.0 * M * N * (double)K);
    if ((ldc & 7) || (N & 7)) return CC_ERR_SHAPE;
    const op16_t* A16;
    const int rca = nt_operand(cx, A, al, bl, M, lda, ldb, K, A16);
    if (rca != CC_OK) return rca;
    EpiBF16 e{C, pre, bias, ldc, M, N, act};
    e.img = Co.img;
    const cc_plan::GemmKnobs& kn = cc_plan::gemm_knobs();
    e.pre_nt = kn.pre_nt;
    switch (cc_plan::pick_bf16out(act, pre != nullptr, e.img, kn)) {
    case cc_plan::EPI_PLAIN: {
        EpiBF16Plain p{C, bias, ldc, M, N};
        return launch_gemm(al, bl, A16, lda, B, ldb, M, N, K, 1, p, st);
    }
    case cc_plan::EPI_SPEC: {
        EpiBF16T<3, 1> g3{C, pre, bias, ldc, M, N, 3};
        return launch_gemm(al, bl, A16, lda, B, ldb, M, N, K, 1, g3, st);
    }
    default: return launch_gemm(al, bl, A16, lda, B, ldb, M, N, K, 1, e, st);
    }
}
}  // namespace CC_NS
