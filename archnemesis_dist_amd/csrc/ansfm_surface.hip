// ansfm_surface.hip -- surface reflection (Surface_0.calc_BRDF, ForwardModel_0.calc_brdf_matrix) of libansfm.so.  gfx950 only.
#include "ansfm_surface_kernels.hip.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

namespace {

// rows of params[npar][nwave] per LowerBoundaryConditionEnum; 0: not a reflecting surface
int brdf_npar(int lowbc) { return lowbc == 1 ? 1 : lowbc == 2 ? 10 : lowbc == 3 ? 2 : 0; }

template <int NACC>
void launch_matrix(ansfm_ctx *ctx, size_t threads, int lowbc, size_t nwave, int nmu, int nphi, int nf, const double *params,
                   const double *ang, const double *azi, const double *wphi, const double *cosk, double *out)
{
    hipLaunchKernelGGL(k_brdf_matrix<NACC>, dim3(nblk(threads, kBrdfBlock)), dim3(kBrdfBlock), 0, ctx->stream, lowbc, nwave, nmu, nphi,
                       nf, params, ang, azi, wphi, cosk, out);
}

}  // namespace

extern "C" {

int ansfm_brdf_last(const ansfm_ctx *ctx, double *kernel_ms)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (kernel_ms) *kernel_ms = ctx->brdf_ms;
    return ANSFM_OK;
}

int ansfm_surface_brdf(ansfm_ctx *ctx, int lowbc, int nwave, const double *params, int ntheta, const double *sol_ang,
                       const double *emiss_ang, const double *azi_ang, double *brdf)
{
    CHECK_CTX(ctx);
    char msg[256];
    const int npar = brdf_npar(lowbc);
    if (!npar) {
        snprintf(msg, sizeof msg, "surface_brdf: lowbc %d is not a reflecting surface (1 LAMBERTIAN, 2 HAPKE, 3 OREN_NAYAR)", lowbc);
        FAIL(ANSFM_ERR_INVALID, msg);
    }
    if (nwave <= 0 || ntheta <= 0 || !params || !sol_ang || !emiss_ang || !azi_ang || !brdf)
        FAIL(ANSFM_ERR_INVALID, "surface_brdf: sizes must be positive and no pointer null");
    const size_t n = (size_t)nwave * ntheta;
    if (n > ((size_t)1 << 36)) FAIL(ANSFM_ERR_INVALID, "surface_brdf: more than 2^36 points; split the wavenumbers");
    HIPCHK(hipSetDevice(ctx->device));
    Stager st{ctx};
    const double *d_par = st.up(params, (size_t)npar * nwave), *d_sol = st.up(sol_ang, ntheta), *d_emi = st.up(emiss_ang, ntheta),
                 *d_azi = st.up(azi_ang, ntheta);
    if (st.rc != ANSFM_OK) return st.rc;
    HIPCHK(ctx->brdf_out.reserve(n * sizeof(double)));
    double *d_out = ctx->brdf_out.as<double>();
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_brdf_points, dim3(nblk(n, kBrdfBlock)), dim3(kBrdfBlock), 0, ctx->stream, lowbc, (size_t)nwave, (size_t)ntheta,
                       d_par, d_sol, d_emi, d_azi, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIPCHK(hipMemcpyAsync(brdf, d_out, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->brdf_ms = ms;
    return ANSFM_OK;
}

int ansfm_brdf_matrix(ansfm_ctx *ctx, int lowbc, int nwave, const double *params, int nmu, const double *ang_deg, int nphi, int nf,
                      const double *azi_deg, const double *phix_deg, const double *wphi, const double *cosk, double *brdf_mat)
{
    CHECK_CTX(ctx);
    char msg[256];
    if (lowbc < 0 || lowbc > 3) {
        snprintf(msg, sizeof msg, "brdf_matrix: lowbc %d is not a LowerBoundaryConditionEnum value (0 .. 3)", lowbc);
        FAIL(ANSFM_ERR_INVALID, msg);
    }
    if (nwave <= 0 || nmu < 1 || nmu > 1024 || nphi < 1 || nphi > (1 << 20) || nf < 0 || !brdf_mat)
        FAIL(ANSFM_ERR_INVALID, "brdf_matrix: nwave >= 1, 1 <= nmu <= 1024, 1 <= nphi <= 2^20, nf >= 0 and a result pointer");
    if (nf > kBrdfMaxNF) {
        snprintf(msg, sizeof msg, "brdf_matrix: nf %d is above the %d Fourier orders that are built", nf, kBrdfMaxNF);
        FAIL(ANSFM_ERR_INVALID, msg);
    }
    const size_t threads = (size_t)nwave * nmu * nmu, n = threads * (nf + 1);
    if (n > ((size_t)1 << 36)) FAIL(ANSFM_ERR_INVALID, "brdf_matrix: more than 2^36 matrix elements; split the wavenumbers");
    if (lowbc == 0 || lowbc == 3) {            // calc_brdf_matrix leaves its zeros for them (:5204-5211)
        memset(brdf_mat, 0, n * sizeof(double));
        ctx->brdf_ms = 0;
        return ANSFM_OK;
    }
    const int nk = nphi + 1;
    if (!params || !ang_deg || !azi_deg || !phix_deg || !wphi || !cosk) FAIL(ANSFM_ERR_INVALID, "brdf_matrix: null pointer");
    for (int k = 0; k < nk; ++k) {            // the exact comparisons of the kernels rest on this table
        const double phi = 180. - azi_deg[k], fold = phi > 180. ? 180. - (phi - 180.) : (phi < 0. ? -phi : phi);
        if (!(phix_deg[k] == fold)) {
            snprintf(msg, sizeof msg, "brdf_matrix: phix[%d] = %.17g is not the fold of 180 - %.17g into [0, 180]", k, phix_deg[k],
                     azi_deg[k]);
            FAIL(ANSFM_ERR_INVALID, msg);
        }
    }
    HIPCHK(hipSetDevice(ctx->device));
    Stager st{ctx};
    const double *d_par = st.up(params, (size_t)brdf_npar(lowbc) * nwave), *d_ang = st.up(ang_deg, nmu), *d_phix = st.up(phix_deg, nk),
                 *d_wphi = st.up(wphi, nk), *d_cosk = st.up(cosk, (size_t)(nf + 1) * nk);
    if (st.rc != ANSFM_OK) return st.rc;
    HIPCHK(ctx->brdf_out.reserve(n * sizeof(double)));
    HIPCHK(ctx->brdf_azi.reserve((size_t)4 * nk * sizeof(double)));
    double *d_out = ctx->brdf_out.as<double>(), *d_azi = ctx->brdf_azi.as<double>();
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_brdf_azimuth, dim3(nblk(nk, kBrdfBlock)), dim3(kBrdfBlock), 0, ctx->stream, nk, d_phix, d_azi);
    const size_t W = nwave;
    if (nf < 1) launch_matrix<1>(ctx, threads, lowbc, W, nmu, nphi, nf, d_par, d_ang, d_azi, d_wphi, d_cosk, d_out);
    else if (nf < 3) launch_matrix<3>(ctx, threads, lowbc, W, nmu, nphi, nf, d_par, d_ang, d_azi, d_wphi, d_cosk, d_out);
    else if (nf < 9) launch_matrix<9>(ctx, threads, lowbc, W, nmu, nphi, nf, d_par, d_ang, d_azi, d_wphi, d_cosk, d_out);
    else if (nf < 17) launch_matrix<17>(ctx, threads, lowbc, W, nmu, nphi, nf, d_par, d_ang, d_azi, d_wphi, d_cosk, d_out);
    else launch_matrix<kBrdfMaxNF + 1>(ctx, threads, lowbc, W, nmu, nphi, nf, d_par, d_ang, d_azi, d_wphi, d_cosk, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIPCHK(hipMemcpyAsync(brdf_mat, d_out, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->brdf_ms = ms;
    return ANSFM_OK;
}

}  // extern "C"
