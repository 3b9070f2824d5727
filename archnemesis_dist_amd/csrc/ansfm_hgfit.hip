// ansfm_hgfit.hip -- double Henyey-Greenstein fit of phase functions (Scatter_0.subfithgm) of libansfm.so.  gfx950 only.
#include "ansfm_hgfit_kernels.hip.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

namespace {
constexpr int kHgFitsMax = 1 << 20;    // fits of one call
}

extern "C" {

int ansfm_hg_fit_last(const ansfm_ctx *ctx, double *kernel_ms)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (kernel_ms) *kernel_ms = ctx->hg_ms;
    return ANSFM_OK;
}

int ansfm_hg_fit(ansfm_ctx *ctx, int nfit, int nphase, const double *theta_deg, const double *phase, double *f, double *g1,
                 double *g2, double *rms, int32_t *counts)
{
    CHECK_CTX(ctx);
    char msg[256];
    if (nfit <= 0 || nfit > kHgFitsMax) {
        snprintf(msg, sizeof msg, "hg_fit: %d fits are outside 1 .. %d", nfit, kHgFitsMax);
        FAIL(ANSFM_ERR_INVALID, msg);
    }
    if (nphase <= 0 || nphase > kHgNphaseCap) {
        snprintf(msg, sizeof msg, "hg_fit: %d angles are outside 1 .. %d", nphase, kHgNphaseCap);
        FAIL(ANSFM_ERR_INVALID, msg);
    }
    if (!theta_deg || !phase || !f || !g1 || !g2 || !rms) FAIL(ANSFM_ERR_INVALID, "hg_fit: a null pointer");
    std::vector<double> h_ca(nphase);
    for (int i = 0; i < nphase; ++i) h_ca[i] = std::cos(theta_deg[i] * M_PI / 180.0);      // subhgphas :2135

    HIPCHK(hipSetDevice(ctx->device));
    // doubles: calpha [nphase] | phase -> log(phase) [nfit][nphase] | f g1 g2 rms [4][nfit]; then counts [nfit][2], fail [nfit]
    const size_t D = sizeof(double), NP = (size_t)nfit * nphase;
    const size_t n_dbl = (size_t)nphase + NP + 4 * (size_t)nfit;
    HIPCHK(ctx->hg_st.reserve(n_dbl * D + 3 * (size_t)nfit * sizeof(int32_t)));
    double *d = ctx->hg_st.as<double>();
    HgFitParams p{};
    p.nfit = nfit; p.nphase = nphase;
    p.calpha = d; p.lphase = d + nphase; p.out = p.lphase + NP;
    p.counts = reinterpret_cast<int32_t *>(p.out + 4 * (size_t)nfit); p.fail = p.counts + 2 * (size_t)nfit;
    HIPCHK(hipMemcpyAsync(d, h_ca.data(), (size_t)nphase * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(p.lphase, phase, NP * D, hipMemcpyHostToDevice, ctx->stream));
    ctx->hg_ms = 0;
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_hg_fit, dim3(nblk(nfit, kHgWaves)), dim3(kHgLanes * kHgWaves), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    std::vector<double> h_out(4 * (size_t)nfit);
    std::vector<int32_t> h_int(3 * (size_t)nfit);
    HIPCHK(hipMemcpyAsync(h_out.data(), p.out, h_out.size() * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_int.data(), p.counts, h_int.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->hg_ms = ms;
    for (int i = 0; i < nfit; ++i)
        if (h_int[2 * (size_t)nfit + i]) {
            snprintf(msg, sizeof msg, "hg_fit: fit %d: the normal equations have a zero pivot (the reference's matrix is singular)", i);
            FAIL(ANSFM_ERR_INVALID, msg);
        }
    const size_t nb = (size_t)nfit * D;
    memcpy(f, h_out.data(), nb); memcpy(g1, h_out.data() + nfit, nb);
    memcpy(g2, h_out.data() + 2 * (size_t)nfit, nb); memcpy(rms, h_out.data() + 3 * (size_t)nfit, nb);
    if (counts) memcpy(counts, h_int.data(), 2 * (size_t)nfit * sizeof(int32_t));
    return ANSFM_OK;
}

}  // extern "C"
