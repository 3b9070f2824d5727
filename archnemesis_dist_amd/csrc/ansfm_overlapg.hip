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
    const long grid = merge_grid(ctx->num_cus, lds, 8, (long)n_models * (Wpad / kWave) * L);
    const int rc = merge_launch_begin(
        ctx, p, grid,
        {{&ctx->scratch, (size_t)6 * (G + 1) * kWave * sizeof(double)},
         {&ctx->gscratch, (3 + 2 * (size_t)NP1) * G * kWave * sizeof(double)},
         {&ctx->perm, (size_t)((G * G + kCodesPerWord - 1) / kCodesPerWord) * kWave * sizeof(unsigned long long)}});
    if (rc) return rc;
    p.scratch = ctx->scratch.as<double>();
    pg.gscratch = ctx->gscratch.as<double>();
    pg.perm = ctx->perm.as<unsigned long long>();
    (void)from_k;                     // the kernel tests p.kin (run-time flag, see load_gas_g)
    using GradKernel = void (*)(OverlapGParams);
    const bool w32 = ctx->delg_f32 != 0;
    const GradKernel kern = by_list_len(G, [&](auto d) -> GradKernel {
        constexpr int D = decltype(d)::value;
        if (w32) return sorted ? k_ck_overlapg<D, true, true> : k_ck_overlapg<D, true, false>;
        return sorted ? k_ck_overlapg<D, false, true> : k_ck_overlapg<D, false, false>;
    });
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, pg);
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

}  // namespace ansfm
