#include "gemm.hip.h"
#include "gemm_api.h"
namespace CC_NS {
int gemm_dact(int al, int bl, ActIn A, int lda, const op16_t* B, int ldb, int M, int N, int K, Act Co, int ldc,
              const act_t* aux, int act, Call& cx) {
    const hipStream_t st = cx.st;
    act_t* const C = Co.p;
    cc_shared::ProfScope _all(cc_shared::SITE_ALL_GEMMS, st, 2.0 * M * N * (double)K);
    if ((ldc & 7) || (N & 7)) return CC_ERR_SHAPE;
    const op16_t* A16;
    const int rca = nt_operand(cx, A, al, bl, M, lda, ldb, K, A16);
    if (rca != CC_OK) return rca;
    EpiDAct e{C, aux, ldc, M, N, act};
    e.img = Co.img;
    if (cc_plan::pick_dact(act, e.img, cc_plan::gemm_knobs()) == cc_plan::EPI_SPEC) {
        EpiDActT<3> m{C, aux, ldc, M, N, 3};
        return launch_gemm(al, bl, A16, lda, B, ldb, M, N, K, 1, m, st);
    }
    return launch_gemm(al, bl, A16, lda, B, ldb, M, N, K, 1, e, st);
}
}  // namespace CC_NS
