// gemm_pp4_ext.hip — the fp8-MFMA and LayerNorm-folding instances of the persistent ping-pong kernel (gemm_pp4.h), called by launch_pp4 (gemm.hip)
// with its grid.  A separate object: these instances take as long to compile as the rest of the GEMM family together.
#include "gemm_pp4.h"

// The fp8-MFMA and LayerNorm-folding instances of the persistent kernel (called by launch_pp4 with its grid).
int launch_pp4_ext(const GemmArgs &g, int grid, hipStream_t s) {
    constexpr int smem = PP4_SMEM;
    if (g.A8 && g.hm_tok) return EILEV_E_UNSUPPORTED;
    if (g.A8) {  // fp8 x fp8 on the fp8 MFMA: byte operands, K halved so that the kernel's 2-byte strides are byte strides
        if (g.epi == 1) return EILEV_E_UNSUPPORTED;
        GemmArgs h = g;
        h.A = reinterpret_cast<const bf16 *>(g.A8);
        h.W = reinterpret_cast<const bf16 *>(g.W8);
        h.K = g.K / 2; h.lda = g.lda / 2; h.ldw = g.ldw / 2;
        return eilev_with_epi<0, 2>(g.epi, [&](auto e) { return GEMM_FORM(4040 + decltype(e)::value), eilev_launch<gemm_pp4_kernel<decltype(e)::value, true>>(dim3(grid), dim3(512), smem, s, h); });
    }
    if (g.hm_tok && !hm_takes(g)) return EILEV_E_UNSUPPORTED;  // head-major q|k|v: the 16 x 16 folded-LayerNorm consumer only (common.h)
    // LayerNorm-folding variants: consumer (qkv, fc1 + GELU) / producer (proj, fc2 with the residual)
    if (g.epi == 2 || g.out_f32 || (g.ln_rows && (g.resid || g.stat_out || !g.ln_csum || ((uintptr_t)g.ln_csum & 15) || ((uintptr_t)g.ln_rows & 7))) ||
        (g.stat_out && (!g.resid || g.epi != 0 || g.stat_ld < g.M || ((uintptr_t)g.stat_out & 7))))
        return EILEV_E_UNSUPPORTED;
    const bool lean = pp4_all_lean(g);  // the 16 x 16 MFMA instances (gemm_pp4.h M16)
    if (g.stat_out)  // statistics producers (ViT proj / fc2)
        return GEMM_FORM(lean ? 4220 : 4200), lean ? eilev_launch<gemm_pp4_kernel<0, false, 2, 2>>(dim3(grid), dim3(512), smem, s, g)
                    : eilev_launch<gemm_pp4_kernel<0, false, 2>>(dim3(grid), dim3(512), smem, s, g);
    return eilev_with_epi<0, 1>(g.epi, [&](auto e) {  // folded-LayerNorm consumers (ViT qkv / fc1)
        constexpr int EPI = decltype(e)::value;
        return GEMM_FORM((lean ? 4110 : 4100) + EPI), lean ? eilev_launch<gemm_pp4_kernel<EPI, false, 1, 1>>(dim3(grid), dim3(512), smem, s, g)
                    : eilev_launch<gemm_pp4_kernel<EPI, false, 1>>(dim3(grid), dim3(512), smem, s, g);
    });
}
