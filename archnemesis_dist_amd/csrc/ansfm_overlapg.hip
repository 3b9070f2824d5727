// ansfm_overlapg.hip -- translation unit of k_ck_overlapg (ansfm_overlapg_kernels.hip.h): the instantiations of the gradient
// merge and their launcher.
#include "ansfm_overlapg_kernels.hip.h"
#include "ansfm_ctx.hip.h"

namespace ansfm {

int launch_overlapg(ansfm_ctx *ctx, bool from_k, const double *kin, const double *dkin, int W, int Wpad,
                    int G, int S, int L, int n_models, const LayerInterp *li, const double *amount,
                    const double *del_g_dev, const double *del_g_host, double *tau, double *dk, bool generic)
{
    OverlapGParams pg;
    memset(&pg, 0, sizeof pg);
    OverlapParams &p = pg.o;
    merge_params(ctx, p, kin, W, Wpad, G, S, L, n_models, li, amount, del_g_dev, del_g_host, tau);
    pg.dkin = dkin;
    pg.dk = dk;
    pg.gas_mask = from_k ? 0xFFFFFFFFu : ctx->grad_gas_mask;      // the array-level seam returns every slot
    const int NP1 = S + 1;
    // the gas selection mask (ansfm_set_gradient_gases) has one bit per gas and bit 31 for temperature
    if (NP1 > 32) FAIL(ANSFM_ERR_UNSUPPORTED, "gradient path supports at most 31 spectroscopic gases");
    // fast path: every k(g) non-decreasing (tables: checked at upload; array-level seam: in the kernel, rerun otherwise)
    const bool sorted = !generic && (from_k || ctx->monotone);
    const size_t lds = (size_t)(2 * G + 1) * kWave * sizeof(double) + (size_t)(2 * kMaxG + 2) * sizeof(double) + kMaxG * sizeof(float) +
                       (sorted ? 0 : (size_t)2 * G * kWave);
    // blocks per CU: by the LDS size as it is (not rounded to the granule), up to 8; ANSFM_WAVES_PER_CU does not apply here
    long grid = 0;
    const int rc = merge_launch_begin(
        ctx, p, lds, 8,
        {{&ctx->scratch, (size_t)6 * (G + 1) * kWave * sizeof(double)},
         {&ctx->gscratch, (3 + 2 * (size_t)NP1) * G * kWave * sizeof(double)},
         {&ctx->perm, (size_t)((G * G + kCodesPerWord - 1) / kCodesPerWord) * kWave * sizeof(unsigned long long)}},
        &grid);
    if (rc) return rc;
    p.scratch = ctx->scratch.as<double>();
    pg.gscratch = ctx->gscratch.as<double>();
    pg.perm = ctx->perm.as<unsigned long long>();
#define LAUNCH_OVG(D, FK)                                                                                           \
    do {                                                                                                            \
        if (ctx->delg_f32) {                                                                                        \
            if (sorted) hipLaunchKernelGGL((k_ck_overlapg<D, true, true>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, pg);   \
            else hipLaunchKernelGGL((k_ck_overlapg<D, true, false>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, pg);         \
        } else {                                                                                                    \
            if (sorted) hipLaunchKernelGGL((k_ck_overlapg<D, false, true>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, pg);  \
            else hipLaunchKernelGGL((k_ck_overlapg<D, false, false>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, pg);        \
        }                                                                                                           \
    } while (0)
#define LAUNCH_OVG_D(FK)                                              \
    switch (merge_list_len(G)) {                                      \
        case 8: LAUNCH_OVG(8, FK); break;                             \
        case 10: LAUNCH_OVG(10, FK); break;                           \
        case 16: LAUNCH_OVG(16, FK); break;                           \
        case 20: LAUNCH_OVG(20, FK); break;                           \
        default: LAUNCH_OVG(32, FK); break;                           \
    }
    (void)from_k;                     // the kernel tests p.kin (run-time flag, see load_gas_g)
    LAUNCH_OVG_D(false);
#undef LAUNCH_OVG_D
#undef LAUNCH_OVG
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

}  // namespace ansfm
