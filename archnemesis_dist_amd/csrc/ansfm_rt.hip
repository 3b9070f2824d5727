// ansfm_rt.hip -- translation unit of the RT kernels of the correlated-k path (ansfm_rt_kernels.hip.h): thermal emission,
// transmission and single scattering, their gradients, and the launchers the entry points of ansfm_api.hip call.
#include "ansfm_rt_kernels.hip.h"
#include "ansfm_ctx.hip.h"

namespace ansfm {

int launch_rt(ansfm_ctx *ctx, const RtParams &p_in, int n_models)
{
    RtParams p = p_in;
    dim3 grid((unsigned)n_models, (unsigned)p.P, (unsigned)(p.Wpad / kWave));
    if (p.Wpad / kWave > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "thermal RT: more than 65535 wavenumber tiles (4.19e6 wavenumbers)");
    if (p.LIMAX > 1500) FAIL(ANSFM_ERR_UNSUPPORTED, "thermal RT: at most 1500 layers along a path");
    if (p.P > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "thermal RT: at most 65535 paths per call");
    ctx->last_rt_shared = 0;
    // single scattering on the vertical opacities (CIRSrad's branch; the array-level seam hands omega in and keeps the run-time mode)
    const bool ss = p.mode == 2 && p.sca && !p.omega;
    // ... with sca / phase by row: builds of their own (SS == 2); a row then carries everything a layer is read from
    const bool ssr = ss && p.ss_by_row;
    if (ssr && (p.rows <= 0 || (p.cont && !p.cont_by_row) || p.emi || p.per_g))
        FAIL(ANSFM_ERR_INVALID, "thermal RT: sca / phase by row go with a continuum by row");
    // a de-duplicated batch (the states of a numerical Jacobian) in thermal emission or single scattering: every state starts
    // each path from the record state 0 left after the last layer the two have in common
    static const bool prefix_off = [] { const char *e = getenv("ANSFM_RT_PREFIX"); return e && e[0] == '0'; }();
    const size_t rec = (size_t)p.P * p.LIMAX * 3 * p.G * p.Wpad * sizeof(double);
    const size_t lds = (size_t)4 * p.LIMAX * sizeof(double);
    const dim3 blk(kWave, kGY);
    if (!prefix_off && n_models >= 4 && n_models <= 65536 && p.tau_slot && (p.mode == 0 || ss) && !p.emi && !p.per_g && rec <= ((size_t)4 << 30)) {
        HIPCHK(ctx->rt_prefix.reserve(rec));
        const bool per_path = ss && !ssr;                    // dense sca / phase: flags per path
        const size_t nl = (size_t)n_models * p.L * (per_path ? p.P : 1), np = (size_t)n_models * p.P;
        const size_t off_j = (nl + 15) & ~(size_t)15;
        HIPCHK(ctx->rt_same.reserve(off_j + np * sizeof(int32_t)));
        unsigned char *same = ctx->rt_same.as<unsigned char>();
        int32_t *jstart = reinterpret_cast<int32_t *>(same + off_j);
        if (per_path)
            hipLaunchKernelGGL(k_rt_same_ss, dim3((unsigned)p.L, (unsigned)(n_models - 1)), dim3(256), 0, ctx->stream, p.L, p.Wpad, p.P,
                               p.tau_slot, p.cont, p.sca, p.phase, same);
        else
            hipLaunchKernelGGL(k_rt_same, dim3((unsigned)p.L, (unsigned)(n_models - 1)), dim3(256), 0, ctx->stream, p.L, p.Wpad, p.tau_slot,
                               p.cont_by_row ? nullptr : p.cont, same);      // a continuum stored by row is the row's
        hipLaunchKernelGGL(k_rt_jstart, dim3((unsigned)np), dim3(64), 0, ctx->stream, n_models, p.L, p.P, p.LIMAX, p.nlayin, p.layinc,
                           p.scale, p.emtemp, same, jstart, per_path ? 1 : 0);
        p.prefix = ctx->rt_prefix.as<double>(); p.jstart = jstart; p.m0 = 0;
        const dim3 g0(1u, grid.y, grid.z), g1((unsigned)(n_models - 1), grid.y, grid.z);
        if (ssr) {
            hipLaunchKernelGGL((k_thermal_rt<false, 1, 2>), g0, blk, lds, ctx->stream, p);
            p.m0 = 1;
            hipLaunchKernelGGL((k_thermal_rt<true, 2, 2>), g1, blk, lds, ctx->stream, p);
        } else if (ss) {
            hipLaunchKernelGGL((k_thermal_rt<false, 1, 1>), g0, blk, lds, ctx->stream, p);
            p.m0 = 1;
            hipLaunchKernelGGL((k_thermal_rt<true, 2, 1>), g1, blk, lds, ctx->stream, p);
        } else {
            hipLaunchKernelGGL((k_thermal_rt<false, 1>), g0, blk, lds, ctx->stream, p);
            p.m0 = 1;
            hipLaunchKernelGGL((k_thermal_rt<true, 2>), g1, blk, lds, ctx->stream, p);
        }
        HIPCHK(hipGetLastError());
        ctx->last_rt_shared = 1;
        return ANSFM_OK;
    }
    if (ssr && n_models >= 4)
        hipLaunchKernelGGL((k_thermal_rt<true, 0, 2>), grid, blk, lds, ctx->stream, p);
    else if (ssr)
        hipLaunchKernelGGL((k_thermal_rt<false, 0, 2>), grid, blk, lds, ctx->stream, p);
    else if (ss && n_models >= 4)
        hipLaunchKernelGGL((k_thermal_rt<true, 0, 1>), grid, blk, lds, ctx->stream, p);
    else if (ss)
        hipLaunchKernelGGL((k_thermal_rt<false, 0, 1>), grid, blk, lds, ctx->stream, p);
    else if (n_models >= 4)
        hipLaunchKernelGGL(k_thermal_rt<true>, grid, blk, lds, ctx->stream, p);
    else
        hipLaunchKernelGGL(k_thermal_rt<false>, grid, blk, lds, ctx->stream, p);
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

int launch_rtg(ansfm_ctx *ctx, const RtGParams &q, int n_models)
{
    dim3 grid((unsigned)n_models, (unsigned)q.r.P, (unsigned)(q.r.Wpad / kWave));
    if (q.r.Wpad / kWave > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "thermal RT: more than 65535 wavenumber tiles (4.19e6 wavenumbers)");
    // reduction buffer [NP1+2][GY][64] doubles: the largest GY that leaves room for one block per CU
    const size_t per_gy = (size_t)(q.NP1 + 2) * kWave * sizeof(double);
    if (16 * per_gy <= 128 * 1024)
        hipLaunchKernelGGL(k_thermal_rtg<16>, grid, dim3(kWave, 16), 16 * per_gy, ctx->stream, q);
    else if (8 * per_gy <= 128 * 1024)
        hipLaunchKernelGGL(k_thermal_rtg<8>, grid, dim3(kWave, 8), 8 * per_gy, ctx->stream, q);
    else
        hipLaunchKernelGGL(k_thermal_rtg<4>, grid, dim3(kWave, 4), 4 * per_gy, ctx->stream, q);
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

void launch_thermal_emission_g_seam(ansfm_ctx *ctx, int ISPACE, int W, int G, int NPAR, int NLAYIN, int NVMR, const double *wave,
                                    const double *tau, const double *dtau, const double *temp, const double *press, double TSURF,
                                    const double *emis, double *o_spec, double *o_dspec, double *o_dts)
{
    hipLaunchKernelGGL(k_thermal_emission_g_seam, dim3(nblk((size_t)W * G, 128)), dim3(128), 0, ctx->stream, ISPACE, W, G, NPAR, NLAYIN,
                       NVMR, wave, tau, dtau, temp, press, TSURF, emis, o_spec, o_dspec, o_dts);
}

void launch_dspec_to_ref(ansfm_ctx *ctx, const double *src, double *dst, int W, int Wpad, int NPAR, int LIMAX, int P,
                         const int32_t *nlayin)
{
    hipLaunchKernelGGL(k_dspec_to_ref, dim3(nblk((size_t)W * NPAR * LIMAX * P, 256)), dim3(256), 0, ctx->stream, src, dst, W, Wpad,
                       NPAR, LIMAX, P, nlayin);
}

}  // namespace ansfm
