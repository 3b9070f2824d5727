// ansfm_mie.hip -- Mie theory over a particle size distribution (Scatter_0.makephase) of libansfm.so.  gfx950 only.
#include "ansfm_mie_kernels.hip.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

namespace {
constexpr int kMieBlockDefault = 512;                  // radii per block
constexpr int kMieCapDefault = 1 << 20;                // radii of an open range before "did not terminate"
constexpr size_t kMieWorkspaceMax = (size_t)1 << 30;   // bytes of D_n and coefficients one block may take
}

extern "C" {

int ansfm_mie_set_radius_block(ansfm_ctx *ctx, int radii)
{
    CHECK_CTX(ctx);
    if (radii < 0 || radii % kMieChunk) FAIL(ANSFM_ERR_INVALID, "mie_set_radius_block: the block is a multiple of 64 radii (0 = default)");
    ctx->mie_block = radii;
    return ANSFM_OK;
}

int ansfm_mie_set_radius_cap(ansfm_ctx *ctx, int radii)
{
    CHECK_CTX(ctx);
    if (radii < 0) FAIL(ANSFM_ERR_INVALID, "mie_set_radius_cap: the cap is a number of radii (0 = default)");
    ctx->mie_cap = radii;
    return ANSFM_OK;
}

int ansfm_mie_last(const ansfm_ctx *ctx, double *kernel_ms, int32_t *blocks, int32_t *block_radii)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (kernel_ms) *kernel_ms = ctx->mie_ms;
    if (blocks) *blocks = ctx->mie_blocks;
    if (block_radii) *block_radii = ctx->mie_block_radii;
    return ANSFM_OK;
}

int ansfm_mie_makephase(ansfm_ctx *ctx, int nwave, const double *wavel_um, int iscat, const double dsize[3], const double rs[3],
                        const double *refindx, int ntheta, const double *theta_deg, double *xscat, double *xext, double *phas,
                        int32_t *n_radii)
{
    CHECK_CTX(ctx);
    char msg[256];
    if (nwave <= 0 || nwave > 65535 || ntheta <= 0 || ntheta > 4096 || !wavel_um || !dsize || !rs || !refindx || !theta_deg ||
        !xscat || !xext || !phas)
        FAIL(ANSFM_ERR_INVALID, "mie_makephase: bad argument");
    if (iscat < 1 || iscat > 4) {
        snprintf(msg, sizeof msg, "mie_makephase: iscat %d is not a Mie case (1 .. 4)", iscat);
        FAIL(ANSFM_ERR_INVALID, msg);
    }
    int n90 = 0;
    std::vector<double> h_in((size_t)3 * nwave + 2 * ntheta);
    double *h_wavel = h_in.data(), *h_ref = h_wavel + nwave, *h_cs = h_ref + 2 * nwave, *h_s2 = h_cs + ntheta;
    for (int j = 0; j < ntheta; ++j) {
        const double th = theta_deg[j];
        if (!(th >= 0.0 && th <= 90.0)) {
            snprintf(msg, sizeof msg, "mie_makephase: scattering angle %g (index %d) is outside [0, 90]", th, j);
            FAIL(ANSFM_ERR_INVALID, msg);
        }
        n90 += th == 90.0;
        // dmie :1472-1485
        if (th == 0.0) { h_cs[j] = 1.0; h_s2[j] = 0.0; }
        else if (th == 90.0) { h_cs[j] = 0.0; h_s2[j] = 1.0; }
        else { h_cs[j] = std::cos(M_PI * th / 180.0); h_s2[j] = 1.0 - h_cs[j] * h_cs[j]; }
    }
    const int nphas = n90 == 1 ? 2 * ntheta - 1 : 2 * ntheta;
    for (int w = 0; w < nwave; ++w) {
        if (!(wavel_um[w] > 0.0) || !std::isfinite(wavel_um[w]) || !std::isfinite(refindx[2 * w]) || !std::isfinite(refindx[2 * w + 1])) {
            snprintf(msg, sizeof msg, "mie_makephase: wavelength %g um (index %d) or its refractive index is not usable", wavel_um[w], w);
            FAIL(ANSFM_ERR_INVALID, msg);
        }
        h_wavel[w] = wavel_um[w]; h_ref[2 * w] = refindx[2 * w]; h_ref[2 * w + 1] = refindx[2 * w + 1];
    }
    if (!(rs[0] > 0.0) || !(rs[2] > 0.0) || !std::isfinite(rs[0]) || !std::isfinite(rs[1]) || !std::isfinite(rs[2]))
        FAIL(ANSFM_ERR_INVALID, "mie_makephase: the first radius rs[0] and the step rs[2] must be positive");
    const int cap = ctx->mie_cap ? ctx->mie_cap : kMieCapDefault;
    const int B = ctx->mie_block ? ctx->mie_block : kMieBlockDefault;

    MieParams p{};
    p.nwave = nwave; p.ntheta = ntheta; p.nphas = nphas; p.iscat = iscat;
    p.d0 = dsize[0]; p.d1 = dsize[1]; p.d2 = dsize[2];
    p.r1 = rs[0]; p.delr = rs[2]; p.sqrt2pi = std::sqrt(2.0 * M_PI);
    if (rs[1] < rs[0]) {              // open range: ends where n Q_sca has fallen to 1e-6 of its maximum beyond r_peak (:1693-1709)
        p.inr = 0; p.mend = cap; p.rmax = 0.0;
        if (dsize[1] != 0.0) {
            if (iscat == 1) p.rmax = dsize[2] * dsize[0] * dsize[1];
            else if (iscat == 2) p.rmax = std::exp(std::log(dsize[0]) - dsize[1] * dsize[1]);
            else if (iscat == 3) p.rmax = std::pow(dsize[0] / (dsize[1] * dsize[2]), 1.0 / dsize[2]);
        }
    } else {                          // closed range (:1683-1685)
        const double q = (rs[1] - rs[0]) / rs[2];
        if (!(q < (double)cap)) {
            snprintf(msg, sizeof msg, "mie_makephase: a closed range of %g radii is above the cap of %d", q + 1.0, cap);
            FAIL(ANSFM_ERR_INVALID, msg);
        }
        int inr = 1 + (int)q;
        if (inr > 1 && inr % 2 != 0) ++inr;
        p.inr = inr; p.mend = inr;
    }

    HIPCHK(hipSetDevice(ctx->device));
    const size_t T = (size_t)nwave * B, D = sizeof(double), NT = (size_t)nwave * (ntheta + 1) * 3;
    if (T > ((size_t)1 << 26)) FAIL(ANSFM_ERR_INVALID, "mie_makephase: wavelengths times the radius block exceed 2^26; set a smaller block");
    // doubles: inputs | qext qsca anr [T] | nqmax [nwave] | partial | total | xscat xext [nwave] phas; then the int arrays
    const size_t n_in = h_in.size(), n_part = (size_t)(B / kMieChunk) * NT;
    const size_t n_dbl = n_in + 3 * T + nwave + n_part + NT + 2 * (size_t)nwave + (size_t)nwave * nphas;
    HIPCHK(ctx->mie_st.reserve(n_dbl * D + (2 * T + 3 * (size_t)nwave) * sizeof(int)));
    double *d = ctx->mie_st.as<double>();
    p.wavel = d; p.refindx = d + nwave; p.cstht = d + 3 * (size_t)nwave; p.si2tht = p.cstht + ntheta; d += n_in;
    p.qext = d; p.qsca = d + T; p.anr = d + 2 * T; d += 3 * T;
    p.nqmax = d; d += nwave;
    p.partial = d; d += n_part;
    p.total = d; d += NT;
    p.xscat = d; p.xext = d + nwave; p.phas = d + 2 * (size_t)nwave; d += 2 * (size_t)nwave + (size_t)nwave * nphas;
    int *di = reinterpret_cast<int *>(d);
    p.nterm = di; p.fail = di + T; p.mcut = di + 2 * T; p.failcode = p.mcut + nwave; p.failm = p.failcode + nwave;
    std::vector<int> h_state((size_t)3 * nwave, 0);
    std::fill(h_state.begin(), h_state.begin() + nwave, INT_MAX);
    HIPCHK(hipMemcpyAsync(const_cast<double *>(p.wavel), h_in.data(), n_in * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(p.mcut, h_state.data(), h_state.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(p.nqmax, 0, (size_t)nwave * D, ctx->stream));
    HIPCHK(hipMemsetAsync(p.total, 0, NT * D, ctx->stream));

    ctx->mie_ms = 0; ctx->mie_blocks = 0; ctx->mie_block_radii = 0;
    // the largest |m| / lambda bounds nmx2 of a block from its last radius
    double mk = 0.0;
    for (int w = 0; w < nwave; ++w)
        mk = std::max(mk, std::sqrt(h_ref[2 * w] * h_ref[2 * w] + h_ref[2 * w + 1] * h_ref[2 * w + 1]) / h_wavel[w]);
    int m0 = 0;
    for (;;) {
        if (m0 >= p.mend) {
            if (p.inr) break;
            snprintf(msg, sizeof msg, "mie_makephase: size integration did not terminate within %d radii", cap);
            FAIL(ANSFM_ERR_INVALID, msg);
        }
        int nrad = B;
        size_t ws = 0;
        int NH = 0;
        for (;;) {
            const int mlast = std::min(m0 + nrad, p.mend) - 1;
            const double t0 = 2.0 * M_PI * (p.r1 + (double)mlast * p.delr) * mk * (1.0 + 1e-9);
            NH = 1.1 * t0 > 150.0 ? (int)std::min(t0, (double)kMieNcap / 1.1) + 2 : 136;   // a radius that gives up at nmx1 stores nothing
            ws = (size_t)NH * 6 * nwave * nrad * D;
            if (ws <= kMieWorkspaceMax || nrad == kMieChunk) break;
            nrad = std::max(kMieChunk, nrad / 2 / kMieChunk * kMieChunk);
        }
        if (ws > kMieWorkspaceMax) FAIL(ANSFM_ERR_UNSUPPORTED, "mie_makephase: size parameters whose series do not fit the workspace");
        HIPCHK(ctx->mie_ws.reserve(ws));
        const size_t Tb = (size_t)nwave * nrad;
        p.m0 = m0; p.nrad = nrad; p.NH = NH;
        p.acap = ctx->mie_ws.as<double>(); p.coef = p.acap + (size_t)NH * 2 * Tb;
        HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
        hipLaunchKernelGGL(k_mie_coeff, dim3(nblk(Tb, 256)), dim3(256), 0, ctx->stream, p);
        hipLaunchKernelGGL(k_mie_cutoff, dim3(nblk(nwave, 64)), dim3(64), 0, ctx->stream, p);
        hipLaunchKernelGGL(k_mie_angles, dim3(nrad / kMieChunk, nwave, nblk(ntheta + 1, kMieAngleWaves)),
                           dim3(kMieChunk * kMieAngleWaves), 0, ctx->stream, p);
        hipLaunchKernelGGL(k_mie_accum, dim3(nblk(NT, 256)), dim3(256), 0, ctx->stream, p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
        HIPCHK(hipMemcpyAsync(h_state.data(), p.mcut, h_state.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        ctx->mie_ms += ms; ctx->mie_blocks += 1; ctx->mie_block_radii = std::max(ctx->mie_block_radii, nrad);
        bool all = true;
        for (int w = 0; w < nwave; ++w) {
            const int code = h_state[nwave + w], m = h_state[2 * (size_t)nwave + w];
            if (code) {
                const char *why = code == 1 ? "the logarithmic derivative would start at order 29999 or above"
                                  : code == 2 ? "the series needs more than nmx2 = max(135, int(|m| x)) terms" : "workspace too small";
                snprintf(msg, sizeof msg, "mie_makephase: wavelength %g um (index %d), radius %g um (index %d): %s", h_wavel[w], w,
                         p.r1 + (double)m * p.delr, m, why);
                FAIL(ANSFM_ERR_INVALID, msg);
            }
            all = all && h_state[w] != INT_MAX;
        }
        if (all) break;
        m0 += nrad;
    }
    hipLaunchKernelGGL(k_mie_finish, dim3(nblk((size_t)nwave * nphas, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(xscat, p.xscat, (size_t)nwave * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(xext, p.xext, (size_t)nwave * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(phas, p.phas, (size_t)nwave * nphas * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (n_radii)
        for (int w = 0; w < nwave; ++w) n_radii[w] = h_state[w] + 1;
    return ANSFM_OK;
}

}  // extern "C"
