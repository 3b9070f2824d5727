// ansfm_phase.hip -- aerosol phase functions on the calculation grid (Scatter_0.calc_phase, calc_phase_ray) of libansfm.so: the
// array-level entries, the resident source on the table's grid and what the fused scattering entries launch.  gfx950 only.
#include "ansfm_phase_kernels.hip.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

namespace {

constexpr size_t D = sizeof(double);

size_t phase_tab_doubles(int imie, int NWS, int NDUST, int NTAB) { return (size_t)(imie == 0 ? 3 : NTAB) * NWS * NDUST; }

// The tables of a call or an upload: sizes, pointers, order.  Launches nothing.
int phase_check_tables(ansfm_ctx *ctx, const std::string &fn, int imie, int NWS, const double *SWAVE, int NDUST, int NTAB,
                       const double *THETA_TAB, const double *tab)
{
    if (imie < 0 || imie > 2) FAIL(ANSFM_ERR_INVALID, fn + "imie must be 0 (Henyey-Greenstein), 1 (tabulated) or 2 (Legendre)");
    if (!SWAVE || !tab || (imie == 1 && !THETA_TAB)) FAIL(ANSFM_ERR_INVALID, fn + "a null pointer");
    if (NWS < 2 || NDUST < 1 || (imie != 0 && NTAB < (imie == 1 ? 2 : 1)))
        FAIL(ANSFM_ERR_INVALID, fn + "NWS >= 2, NDUST >= 1, NTAB >= 1 (>= 2 tabulated angles) are needed");
    for (int i = 1; i < NWS; ++i)
        if (!(SWAVE[i] > SWAVE[i - 1])) FAIL(ANSFM_ERR_INVALID, fn + "Scatter.WAVE must be strictly ascending");
    if (imie == 1)
        for (int i = 1; i < NTAB; ++i)
            if (!(THETA_TAB[i] > THETA_TAB[i - 1])) FAIL(ANSFM_ERR_INVALID, fn + "Scatter.THETA must be strictly ascending");
    return ANSFM_OK;
}

// calc_phase's range test (:790) of the W wavenumbers x against the aerosol grid
int phase_check_range(ansfm_ctx *ctx, const std::string &fn, int NWS, const double *SWAVE, int W, const double *x)
{
    double xmin = x[0], xmax = x[0];
    for (int w = 1; w < W; ++w) { xmin = std::min(xmin, x[w]); xmax = std::max(xmax, x[w]); }
    const double rel = 1.0e-6;
    if (SWAVE[0] > (1.0 + rel) * xmin || SWAVE[NWS - 1] < (1.0 - rel) * xmax || xmin != xmin || xmax != xmax)
        FAIL(ANSFM_ERR_INVALID, fn + "the aerosol wavelength range does not fully cover the calculation wavelength range");
    return ANSFM_OK;
}

// interp1d(THETA, PHASE, axis=1) has bounds_error on
int phase_check_angles(ansfm_ctx *ctx, const std::string &fn, int imie, int NTAB, const double *THETA_TAB, int nth,
                       const double *theta_deg)
{
    if (imie != 1) return ANSFM_OK;
    for (int t = 0; t < nth; ++t)
        if (!(theta_deg[t] >= THETA_TAB[0] && theta_deg[t] <= THETA_TAB[NTAB - 1]))
            FAIL(ANSFM_ERR_INVALID, fn + "angle " + std::to_string(t) + " is outside the tabulated angles (interp1d: out of the interpolation range)");
    return ANSFM_OK;
}

// Cuts a buffer into arrays of doubles and, behind them, of int32
struct Carve {
    double *d;
    template <class T = double> T *take(size_t n)
    {
        T *r = reinterpret_cast<T *>(d);
        d += (n * sizeof(T) + D - 1) / D;
        return r;
    }
};

void phase_launch_fn(ansfm_ctx *ctx, const PhaseParams &p, bool scat)
{
    const unsigned grid = nblk((size_t)p.W * p.nth, kPhaseBlock);
    if (scat) hipLaunchKernelGGL(k_phase_fn<true>, dim3(grid), dim3(kPhaseBlock), 0, ctx->stream, p);
    else hipLaunchKernelGGL(k_phase_fn<false>, dim3(grid), dim3(kPhaseBlock), 0, ctx->stream, p);
}

// p for the resident source: tables, grid and brackets
PhaseParams phase_source_params(ansfm_ctx *ctx)
{
    PhaseParams p;
    memset(&p, 0, sizeof p);
    p.imie = ctx->phase_imie; p.NWS = ctx->phase_NWS; p.NDUST = ctx->phase_n; p.NTAB = ctx->phase_NTAB;
    p.W = ctx->W; p.Wpad = ctx->Wpad;
    Carve c{ctx->phase_src.as<double>()};
    p.swave = c.take(p.NWS); p.theta_tab = c.take(p.imie == 1 ? p.NTAB : 0);
    p.tab = c.take(phase_tab_doubles(p.imie, p.NWS, p.NDUST, p.NTAB));
    p.xlo = c.take(p.W); p.xhi = c.take(p.W);
    p.hg = c.take(p.imie == 0 ? (size_t)3 * p.NDUST * p.Wpad : 0);
    p.wlo = c.take<int32_t>(p.W);
    p.x = ctx->d_wave.as<double>();
    return p;
}

}  // namespace

namespace ansfm {

int phase_source_check(ansfm_ctx *ctx, const std::string &fn, int ncont)
{
    if (!ctx->phase_n) FAIL(ANSFM_ERR_INVALID, fn + "no phase-function source on this table's grid (ansfm_upload_phase after the table)");
    if (ctx->phase_n != ncont)
        FAIL(ANSFM_ERR_INVALID, fn + "ncont = " + std::to_string(ncont) + ", the phase-function source has " +
                                    std::to_string(ctx->phase_n) + " populations");
    return ANSFM_OK;
}

int phase_source_angles(ansfm_ctx *ctx, const std::string &fn, int nth, const double *theta_deg)
{
    if (nth < 1 || !theta_deg) FAIL(ANSFM_ERR_INVALID, fn + "at least one angle is needed");
    return phase_check_angles(ctx, fn, ctx->phase_imie, ctx->phase_NTAB, ctx->phase_h_theta.data(), nth, theta_deg);
}

int launch_phase_source(ansfm_ctx *ctx, int nth, const double *theta_deg, const double *mu_theta, int ray, double *out)
{
    const bool scat = mu_theta != nullptr;
    PhaseParams p = phase_source_params(ctx);
    HIPCHK(ctx->phase_ws.reserve((3 * (size_t)nth + 1) * D + (size_t)nth * sizeof(int32_t)));
    Carve c{ctx->phase_ws.as<double>()};
    double *d_theta = c.take(nth), *d_mu = c.take(nth);
    p.ca = c.take(nth); p.tlo = c.take<int32_t>(nth);
    p.nth = nth; p.theta = d_theta; p.mu = d_mu;
    p.out = out; p.ostride = p.NDUST + (ray ? 1 : 0); p.ray = ray;
    HIPCHK(hipMemcpyAsync(d_theta, theta_deg, (size_t)nth * D, hipMemcpyHostToDevice, ctx->stream));
    if (scat) HIPCHK(hipMemcpyAsync(d_mu, mu_theta, (size_t)nth * D, hipMemcpyHostToDevice, ctx->stream));
    if (!(scat && p.imie == 0)) {
        hipLaunchKernelGGL(k_phase_prep, dim3(nblk((size_t)nth, kPhaseBlock)), dim3(kPhaseBlock), 0, ctx->stream, p, 0);
        HIPCHK(hipGetLastError());
    }
    phase_launch_fn(ctx, p, scat);
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

}  // namespace ansfm

extern "C" {

int ansfm_phase_last(const ansfm_ctx *ctx, double *kernel_ms)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (kernel_ms) *kernel_ms = ctx->phase_ms;
    return ANSFM_OK;
}

int ansfm_phase_source_info(const ansfm_ctx *ctx, int *imie, int *NDUST)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (imie) *imie = ctx->phase_n ? ctx->phase_imie : -1;
    if (NDUST) *NDUST = ctx->phase_n;
    return ANSFM_OK;
}

int ansfm_calc_phase(ansfm_ctx *ctx, int imie, int NWS, const double *SWAVE, int NDUST, int NTAB, const double *THETA_TAB,
                     const double *tab, int nth, const double *theta_deg, int W, const double *WAVEC, double *phase)
{
    CHECK_CTX(ctx);
    const std::string fn = "calc_phase: ";
    int rc;
    if ((rc = phase_check_tables(ctx, fn, imie, NWS, SWAVE, NDUST, NTAB, THETA_TAB, tab))) return rc;
    if (nth < 1 || W < 1 || !theta_deg || !WAVEC || !phase) FAIL(ANSFM_ERR_INVALID, fn + "a null pointer, no angle or no wavenumber");
    if ((size_t)W * nth * NDUST > ((size_t)1 << 31)) FAIL(ANSFM_ERR_UNSUPPORTED, fn + "more than 2^31 values in one call");
    if ((rc = phase_check_angles(ctx, fn, imie, NTAB, THETA_TAB, nth, theta_deg)) ||
        (rc = phase_check_range(ctx, fn, NWS, SWAVE, W, WAVEC)))
        return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t ntab = phase_tab_doubles(imie, NWS, NDUST, NTAB), nang = imie == 1 ? NTAB : 0, nout = (size_t)W * nth * NDUST;
    HIPCHK(ctx->phase_call.reserve((NWS + nang + ntab + 3 * (size_t)W + 2 * (size_t)nth + nout + 2) * D +
                                   ((size_t)W + nth) * sizeof(int32_t)));
    PhaseParams p;
    memset(&p, 0, sizeof p);
    p.imie = imie; p.NWS = NWS; p.NDUST = NDUST; p.NTAB = NTAB; p.nth = nth; p.W = W; p.Wpad = W;
    Carve c{ctx->phase_call.as<double>()};
    double *d_swave = c.take(NWS), *d_ttab = c.take(nang), *d_tab = c.take(ntab), *d_x = c.take(W), *d_theta = c.take(nth);
    p.swave = d_swave; p.theta_tab = d_ttab; p.tab = d_tab; p.x = d_x; p.theta = d_theta;
    p.xlo = c.take(W); p.xhi = c.take(W); p.ca = c.take(nth); p.out = c.take(nout);
    p.wlo = c.take<int32_t>(W); p.tlo = c.take<int32_t>(nth);
    p.ostride = NDUST; p.ray = 0;
    HIPCHK(hipMemcpyAsync(d_swave, SWAVE, (size_t)NWS * D, hipMemcpyHostToDevice, ctx->stream));
    if (nang) HIPCHK(hipMemcpyAsync(d_ttab, THETA_TAB, nang * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_tab, tab, ntab * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_x, WAVEC, (size_t)W * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_theta, theta_deg, (size_t)nth * D, hipMemcpyHostToDevice, ctx->stream));
    ctx->phase_ms = 0;
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_phase_prep, dim3(nblk((size_t)std::max(W, nth), kPhaseBlock)), dim3(kPhaseBlock), 0, ctx->stream, p, 1);
    HIPCHK(hipGetLastError());
    phase_launch_fn(ctx, p, false);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIPCHK(hipMemcpyAsync(phase, p.out, nout * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->phase_ms = ms;
    return ANSFM_OK;
}

int ansfm_calc_phase_ray(ansfm_ctx *ctx, int nth, const double *theta_deg, double *phase)
{
    CHECK_CTX(ctx);
    if (nth < 1 || !theta_deg || !phase) FAIL(ANSFM_ERR_INVALID, "calc_phase_ray: a null pointer or no angle");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ctx->phase_call.reserve(2 * (size_t)nth * D));
    double *d = ctx->phase_call.as<double>();
    HIPCHK(hipMemcpyAsync(d, theta_deg, (size_t)nth * D, hipMemcpyHostToDevice, ctx->stream));
    ctx->phase_ms = 0;
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_phase_ray, dim3(nblk((size_t)nth, kPhaseBlock)), dim3(kPhaseBlock), 0, ctx->stream, nth, d, d + nth);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIPCHK(hipMemcpyAsync(phase, d + nth, (size_t)nth * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->phase_ms = ms;
    return ANSFM_OK;
}

int ansfm_upload_phase(ansfm_ctx *ctx, int imie, int NWS, const double *SWAVE, int NDUST, int NTAB, const double *THETA_TAB,
                       const double *tab)
{
    CHECK_CTX(ctx);
    const std::string fn = "upload_phase: ";
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, fn + "upload a table first (the source lives on its wavenumber grid)");
    int rc;
    if ((rc = phase_check_tables(ctx, fn, imie, NWS, SWAVE, NDUST, NTAB, THETA_TAB, tab))) return rc;
    if (NDUST > 7) FAIL(ANSFM_ERR_UNSUPPORTED, fn + "more than 7 aerosol populations (as ansfm_upload_dust; use ansfm_calc_phase)");
    const int W = ctx->W, Wpad = ctx->Wpad;
    if ((rc = phase_check_range(ctx, fn, NWS, SWAVE, W, ctx->h_wave.data()))) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t ntab = phase_tab_doubles(imie, NWS, NDUST, NTAB), nang = imie == 1 ? NTAB : 0;
    const size_t nhg = imie == 0 ? (size_t)3 * NDUST * Wpad : 0;
    ctx->phase_n = 0;
    HIPCHK(ctx->phase_src.reserve((NWS + nang + ntab + 2 * (size_t)W + nhg + 1) * D + (size_t)W * sizeof(int32_t)));
    ctx->phase_imie = imie; ctx->phase_NWS = NWS; ctx->phase_NTAB = imie == 0 ? 0 : NTAB; ctx->phase_n = NDUST;
    PhaseParams p = phase_source_params(ctx);
    ctx->phase_n = 0;                                               // until the source stands
    HIPCHK(hipMemcpyAsync(const_cast<double *>(p.swave), SWAVE, (size_t)NWS * D, hipMemcpyHostToDevice, ctx->stream));
    if (nang) HIPCHK(hipMemcpyAsync(const_cast<double *>(p.theta_tab), THETA_TAB, nang * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(const_cast<double *>(p.tab), tab, ntab * D, hipMemcpyHostToDevice, ctx->stream));
    p.nth = 0;
    hipLaunchKernelGGL(k_phase_prep, dim3(nblk((size_t)W, kPhaseBlock)), dim3(kPhaseBlock), 0, ctx->stream, p, 1);
    HIPCHK(hipGetLastError());
    if (imie == 0) {
        hipLaunchKernelGGL(k_phase_hg_grid, dim3(nblk((size_t)Wpad, kPhaseBlock), (unsigned)NDUST, 3), dim3(kPhaseBlock), 0, ctx->stream,
                           p, const_cast<double *>(p.hg));
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));                     // the caller's arrays are free again
    ctx->phase_h_theta.assign(THETA_TAB, THETA_TAB + nang);
    ctx->phase_n = NDUST;
    return ANSFM_OK;
}

int ansfm_phase_from_source(ansfm_ctx *ctx, int nth, const double *theta_deg, double *phase)
{
    CHECK_CTX(ctx);
    const std::string fn = "phase_from_source: ";
    if (!ctx->phase_n) FAIL(ANSFM_ERR_INVALID, fn + "no phase-function source on this table's grid (ansfm_upload_phase after the table)");
    if (!phase) FAIL(ANSFM_ERR_INVALID, fn + "a null pointer");
    int rc;
    if ((rc = phase_source_angles(ctx, fn, nth, theta_deg))) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nout = (size_t)ctx->W * nth * ctx->phase_n;
    HIPCHK(ctx->phase_call.reserve(nout * D));
    ctx->phase_ms = 0;
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    if ((rc = launch_phase_source(ctx, nth, theta_deg, nullptr, 0, ctx->phase_call.as<double>()))) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIPCHK(hipMemcpyAsync(phase, ctx->phase_call.p, nout * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->phase_ms = ms;
    return ANSFM_OK;
}

int ansfm_phasarr_from_source(ansfm_ctx *ctx, int nth, const double *theta_deg, const double *mu_theta, double *phasarr)
{
    CHECK_CTX(ctx);
    const std::string fn = "phasarr_from_source: ";
    if (!ctx->phase_n) FAIL(ANSFM_ERR_INVALID, fn + "no phase-function source on this table's grid (ansfm_upload_phase after the table)");
    if (!phasarr || !mu_theta || nth < 3) FAIL(ANSFM_ERR_INVALID, fn + "a null pointer or fewer than three angles");
    int rc;
    if ((rc = phase_source_angles(ctx, fn, nth, theta_deg))) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nout = (size_t)ctx->phase_n * ctx->W * 2 * nth;
    HIPCHK(ctx->phase_call.reserve(nout * D));
    if ((rc = launch_phase_source(ctx, nth, theta_deg, mu_theta, 0, ctx->phase_call.as<double>()))) return rc;
    HIPCHK(hipMemcpyAsync(phasarr, ctx->phase_call.p, nout * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

}  // extern "C"
