// ansfm_scatter.hip -- multiple scattering of libansfm.so: the scloud11wave core, CIRSrad's scattering branch and its batch.
// gfx950 only.
#include "ansfm_ms_kernels.hip.h"
#include "ansfm_ms_lane.hip.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

extern "C" {

/* ------------------------------------------------------------------------------------------ */
/* multiple scattering                                                                         */
/* ------------------------------------------------------------------------------------------ */
// Switches of the scattering entry points, read once at the top of every call (the tests flip them between calls on one engine):
//   ANSFM_MS_PAD16=0        7 .. 15 streams on the run-time LDS kernels instead of the padded 16-stream ones (ms_setup)
//   ANSFM_MS_WINDOW=<n>     G = 1: n wavenumbers per window of phase matrices and Hansen factors (ms_window_size)
//   ANSFM_MS_PHASE_LDS=1    16 streams, one model per call: k_ms_chain16<true> (phase matrices in LDS, <= 2 components)
//   ANSFM_MS_LANE=0         4 .. 6 streams: the wavefront-per-chain kernel instead of the lane kernel
//   ANSFM_MS_LAYER_CACHE=0  the batch model by model, without the layer cache
//   ANSFM_MS_PREFIX=0       the batch: every model's adding sweep starts at the first layer
//   ANSFM_MS_SLAB=<n>       the batch: at most n wavenumbers per slab (rounded up to tiles of 64 below 16 streams)
//   ANSFM_MS_CHUNK=<n>      the batch: at most n models per launch of the cached chains
struct MsKnobs {
    bool pad16, phase_lds, lane, layer_cache, prefix;
    long window, slab;                                          // 0: not set
    int chunk;
    MsKnobs()
    {
        const char *e;
        pad16 = !((e = getenv("ANSFM_MS_PAD16")) && e[0] == '0');
        window = (e = getenv("ANSFM_MS_WINDOW")) ? std::max(0L, atol(e)) : 0;
        phase_lds = (e = getenv("ANSFM_MS_PHASE_LDS")) && atoi(e) != 0;
        lane = !((e = getenv("ANSFM_MS_LANE")) && e[0] == '0');
        layer_cache = !((e = getenv("ANSFM_MS_LAYER_CACHE")) && atoi(e) == 0);
        prefix = !((e = getenv("ANSFM_MS_PREFIX")) && atoi(e) == 0);
        slab = (e = getenv("ANSFM_MS_SLAB")) ? std::max(0L, atol(e)) : 0;
        chunk = (e = getenv("ANSFM_MS_CHUNK")) ? std::max(0, atoi(e)) : 0;
    }
};

// The arguments of a scattering entry point (include/ansfm.h).  One model per call: n_models = 1, SPEC_G optional; the batch:
// SPEC_G = nullptr, and the context's table is the slice [w_begin, w_begin + ctx->W) of a W_full axis (phasarr covers W_full,
// every other per-wavenumber input and SPECOUT the slice; W_full = ctx->W, w_begin = 0: the whole axis).
struct MsCall {
    int ISPACE, n_models, L;
    const double *lay_press_pa, *lay_temp, *amount, *taucia, *taudust, *tauray, *tauscat;
    int ncont, nth; const double *phasarr, *lfrac, *radg;
    int ngeom; const double *sol_angs, *emiss_angs, *aphis, *solar;
    int lowbc; const double *brdf_matrix; int nmu; const double *mu1, *wt1;
    int nf, nphi, iray, imie; const double *xfac;
    double *SPECOUT, *SPEC_G;
    int W_full, w_begin;
    // the continuum once per distinct layer (ansfm_cirsrad_ck_scatter_batch_rows): cont_row [n][L] into R rows; taucia / taudust /
    // tauray / tauscat are then [R][W] and lfrac [R][ncont][W].  cont_row = nullptr: the dense arrays
    int R; const int32_t *cont_row;
    // the continuum formed inside the call from the context's resident sources, once per distinct layer
    // (ansfm_cirsrad_ck_scatter_batch_cont): the per-layer arrays [n][L] / [n][L][NVMR | ncont | 4] behind it, host pointers,
    // as fused_cont_check left them; taucia .. tauscat, lfrac and cont_row are null
    int fused; ContCall cont;
    // phasarr formed on the device from the resident phase-function source (ansfm_cirsrad_ck_scatter_batch_src): Scatter.THETA
    // in degrees and its cosines [nth], host pointers; phasarr is null
    const double *theta_deg, *mu_theta;
    // per-model phase functions (ansfm_set_phase_variants): the setting this call consumes, validated by the batch entry; null: none
    const MsVariantSet *pv;
};

// The pending per-model phase functions leave the context with the batched call that meets them, whatever becomes of that call
static MsVariantSet ms_take_variants(ansfm_ctx *ctx)
{
    MsVariantSet s = std::move(ctx->ms_pv);
    ctx->ms_pv = MsVariantSet();
    return s;
}

// one model's continuum already on the device, [W][L] / [W][ncont][L] (null = zeros): cirsrad_ck_scatter_impl stages none then
struct MsDevCont { const double *cia, *dust, *ray, *sca, *lf; };

static int ms_check(ansfm_ctx *ctx, const MsCall &c, const char *fn)
{
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, std::string(fn) + ": upload a k-table first");
    if (c.n_models <= 0 || c.L <= 0 || !c.lay_press_pa || !c.lay_temp || !c.amount || c.ncont < 0 || c.ngeom <= 0 || c.nmu < 2 ||
        c.nf < 0 || c.nphi <= 0 || !c.radg || !c.sol_angs || !c.emiss_angs || !c.aphis || !c.solar || !c.brdf_matrix || !c.mu1 ||
        !c.wt1 || !c.SPECOUT || (c.ISPACE != 0 && c.ISPACE != 1) || (c.ncont > 0 && ((!c.phasarr && !c.theta_deg) || (!c.lfrac && !c.fused) || c.nth < 3)))
        FAIL(ANSFM_ERR_INVALID, std::string(fn) + ": bad argument");
    return ANSFM_OK;
}

// The chain kernels: one lane per chain with the matrices in registers (ansfm_ms_lane.hip.h; 4 .. 6 streams), one wavefront per
// chain on LDS matrices (any other stream count), or the matrix-core chain of 16 streams (7 .. 15 padded to it).
enum class MsChain { lane, wavefront, mfma16 };
struct MsRoute { MsChain chain; int ncomp_run; };               // ncomp_run: scattering components in use (aerosols, Rayleigh)

// p for one model over the whole axis of nwave wavenumbers, ng g-ordinates and nlay layers: sizes, quadrature, angles, look-up
// geometry; the per-call limits; the kernels that run it.  Leaves every device pointer null.
// 7 .. 15 streams run on the 16-stream kernels (matrix-core chain, its layer cache, its walk) with the quadrature padded:
// mu = 1 / weight = 0 beyond it, phase matrices, surface operator and boundary radiance zero there, so that every operator is
// block diagonal and the quadrature's block never sees the rest.  The run-time LDS kernels those sizes used to take need
// 1.6 s for the C4 configuration at 12 streams / NF 2, the padded path 0.2 s.  p.nmu_real != 0: padded (ms_pad_inputs).
static int ms_setup(ansfm_ctx *ctx, MsParams &p, const MsCall &c, int nwave, int ng, int nlay, const MsKnobs &kn, MsRoute &r)
{
    if (c.nmu > kMsMaxMu || c.ngeom > kMsMaxPath || c.ncont > 60)
        FAIL(ANSFM_ERR_UNSUPPORTED, "scloud11wave_core: nmu <= 32, npath <= 16 per call supported");
    int nless = 0, nmore = 0;
    for (int i = 0; i < c.ngeom; ++i) { if (c.emiss_angs[i] < 90) ++nless; if (c.emiss_angs[i] > 90) ++nmore; }
    if (nless != c.ngeom && nmore != c.ngeom)
        FAIL(ANSFM_ERR_INVALID, "Emission angles are a mix of values above and below 90 degrees.");   // :776
    const int nmu_in = c.nmu;                                   // the quadrature's size
    const bool pad16 = kn.pad16 && nmu_in >= 7 && nmu_in <= 15;
    const int nmu = pad16 ? 16 : nmu_in;
    memset(&p, 0, sizeof p);
    p.ncont = c.ncont; p.ncomp = c.ncont + 1; p.nwave = nwave; p.nth = c.nth; p.ngeom = c.ngeom; p.lowbc = c.lowbc; p.nmu = nmu;
    p.nmu_real = pad16 ? nmu_in : 0;
    p.nf = c.nf; p.ng = ng; p.nlay = nlay; p.nphi = c.nphi; p.iray = c.iray; p.imie = c.imie;
    p.lookup = (nmore == c.ngeom) ? 1 : 0;
    p.w0 = 0; p.wcount = nwave; p.m0 = 0; p.n_launch = 1;      // one model, the whole spectral axis
    double xs = 0.0;
    for (int k = 0; k < nmu_in; ++k) { xs += c.mu1[k] * c.wt1[k]; p.mu[k] = c.mu1[nmu_in - 1 - k]; p.wtmu[k] = c.wt1[nmu_in - 1 - k]; }
    for (int k = nmu_in; k < nmu; ++k) { p.mu[k] = 1.0; p.wtmu[k] = 0.0; }
    p.xfac = 0.5 / xs;                                          // :720-722
    for (int k = 0; k < c.ngeom; ++k) { p.sol_ang[k] = c.sol_angs[k]; p.emiss_ang[k] = c.emiss_angs[k]; p.aphi[k] = c.aphis[k]; }
    p.ig0 = 0; p.ng_launch = ng;
    p.pw0 = 0; p.nwin = nwave; p.carry_in = 0; p.carry = nullptr;      // one window: the whole axis
    p.phase_tab = (size_t)(c.nf + 2) * (c.nphi + 1) * sizeof(double) <= 48 * 1024 ? 1 : 0;   // cos(ic phi_k) of every order / point
    p.hansen_comp0 = 0;
    r.chain = nmu == 16 ? MsChain::mfma16 : (kn.lane && nmu >= 4 && nmu <= 6) ? MsChain::lane : MsChain::wavefront;
    r.ncomp_run = c.ncont + (c.iray > 0 ? 1 : 0);
    return ANSFM_OK;
}

// radg [rows][nmu] and brdf [W][nmu][nmu][nf + 1] (device) -> the padded copies the 16-stream kernels read
static int ms_pad_inputs(ansfm_ctx *ctx, int nmu, size_t radg_rows, size_t W, int nf, const double **radg, const double **brdf)
{
    const size_t D = sizeof(double);
    HIPCHK(ctx->ms_radg16.reserve(radg_rows * 16 * D));
    HIPCHK(ctx->ms_brdf16.reserve(W * 256 * (nf + 1) * D));
    hipLaunchKernelGGL(k_ms_pad_radg, dim3(nblk(radg_rows * 16, 256)), dim3(256), 0, ctx->stream, radg_rows, nmu, *radg,
                       ctx->ms_radg16.as<double>());
    hipLaunchKernelGGL(k_ms_pad_brdf, dim3(nblk(W * 256 * (size_t)(nf + 1), 256)), dim3(256), 0, ctx->stream, W, nmu, nf + 1, *brdf,
                       ctx->ms_brdf16.as<double>());
    HIPCHK(hipGetLastError());
    *radg = ctx->ms_radg16.as<double>(); *brdf = ctx->ms_brdf16.as<double>();
    return ANSFM_OK;
}

// the chain kernels read TAURAY per (wavenumber, layer) even when there is none: then zeros of WL doubles in ctx->cont_t
static int ms_zero_tauray(ansfm_ctx *ctx, size_t WL, const double **tauray)
{
    if (*tauray) return ANSFM_OK;
    HIPCHK(ctx->cont_t.reserve(WL * sizeof(double)));
    HIPCHK(hipMemsetAsync(ctx->cont_t.p, 0, WL * sizeof(double), ctx->stream));
    *tauray = ctx->cont_t.as<double>();
    return ANSFM_OK;
}

// G = 1 (LBL tables, or a k-table of one g-ordinate): wavenumbers per window of phase matrices and Hansen factors.  The larger
// of 4096 and W / 16, in tiles of 64 (the lane kernels'), at most what keeps one window's buffers under kMsWindowBudget;
// ANSFM_MS_WINDOW overrides (tests, A/B timing).  >= W: one window, the schedule of a single g-ordinate.
static const size_t kMsWindowBudget = (size_t)2 << 30;
static long ms_window_size(long W, int nf, int ncomp, int nmu, const MsKnobs &kn)
{
    const size_t per_w = (size_t)(2 * (nf + 1) + 1) * ncomp * nmu * nmu * sizeof(double);   // ppl + pmi + fc of one wavenumber
    long nwin = std::max<long>(4096, (W + 15) / 16);
    nwin = (nwin + 63) / 64 * 64;
    nwin = std::min(nwin, std::max<long>(64, (long)(kMsWindowBudget / per_w) / 64 * 64));
    if (kn.window) nwin = kn.window;
    return std::min(nwin, W);
}

// the walk's kernel by quadrature size: 16 (the matrix-core chain's), 5 (the reference's default, Scatter_0.py:59), 4, 6, 8;
// any other size takes the run-time build.  One block per scattering component in use.
static void ms_launch_hansen(hipStream_t st, const MsParams &pp)
{
    const dim3 hg((unsigned)(pp.pairs ? pp.npairs : pp.ncont + (pp.iray > 0 ? 1 : 0))), hb(64);   // pairs: one block per (variant, component)
    switch (pp.nmu) {
    case 16: hipLaunchKernelGGL(k_ms_hansen_seq<16>, hg, hb, 0, st, pp); break;
    case 4: hipLaunchKernelGGL(k_ms_hansen_seq<4>, hg, hb, 0, st, pp); break;
    case 5: hipLaunchKernelGGL(k_ms_hansen_seq<5>, hg, hb, 0, st, pp); break;
    case 6: hipLaunchKernelGGL(k_ms_hansen_seq<6>, hg, hb, 0, st, pp); break;
    case 8: hipLaunchKernelGGL(k_ms_hansen_seq<8>, hg, hb, 0, st, pp); break;
    default: hipLaunchKernelGGL(k_ms_hansen_seq<0>, hg, hb, 0, st, pp); break;
    }
}

// phase matrices of the wavenumbers [pw.pw0, pw.pw0 + pw.nwin) (Rayleigh in slot ncont even when there are no aerosols)
static void ms_launch_phase(hipStream_t st, const MsParams &pw)
{
    const size_t lds = pw.phase_tab ? (size_t)(pw.nf + 2) * (pw.nphi + 1) * sizeof(double) : 0;
    if (pw.pairs) {                                             // every (variant, component) pair, Rayleigh among them, in one launch
        if (pw.npairs > 0) hipLaunchKernelGGL(k_ms_phase, dim3((unsigned)pw.nwin, (unsigned)pw.npairs), dim3(256), lds, st, pw);
        return;
    }
    if (pw.ncont > 0) hipLaunchKernelGGL(k_ms_phase, dim3((unsigned)pw.nwin, (unsigned)pw.ncont), dim3(256), lds, st, pw);
    if (pw.iray > 0) {
        MsParams pr = pw;
        pr.phase_comp0 = pw.ncont;
        hipLaunchKernelGGL(k_ms_phase, dim3((unsigned)pw.nwin, 1), dim3(256), lds, st, pr);
    }
}

}  // extern "C": the chain launcher is a template
// The chains of p.wcount wavenumbers from p.w0, p.ng_launch g-ordinates from p.ig0 and, CACHE = 2, the p.n_launch models from
// p.m0.  CACHE: 0 one model per call; 1 the batch's model 0, which fills the layer cache; 2 the other models over it.
// Instantiates k_ms_chain_lane<4|5|6, CACHE>, k_ms_chain<5|8|0, CACHE>, k_ms_chain16<false, CACHE> and k_ms_chain16<true, 0>.
template <int CACHE> static int ms_launch_chain(ansfm_ctx *ctx, MsChain k, hipStream_t st, const MsParams &p)
{
    // one block per (wavenumber, g) on the matrix cores, which work through the Fourier orders themselves; per (wavenumber, g,
    // order) on a wavefront; per (tile of 64 wavenumbers, g, order) on lanes.  16 streams, CACHE = 2: a model's blocks rounded
    // up to 8.
    size_t grid = (k == MsChain::lane ? ((size_t)p.wcount + 63) / 64 : (size_t)p.wcount) * p.ng_launch;
    if (k != MsChain::mfma16) grid *= p.nf + 1;
    if (CACHE == 2) {
        grid = (k == MsChain::mfma16 ? (grid + 7) / 8 * 8 : grid) * p.n_launch;
        if (grid > 0x7FFFFFFFull) FAIL(ANSFM_ERR_UNSUPPORTED, "cirsrad_ck_scatter_batch: slab x models too large for one launch");
    }
    const size_t D = sizeof(double), nn = (size_t)p.nmu * p.nmu;
    const dim3 g((unsigned)grid), b(64);
    if (k == MsChain::lane) {
        const size_t lds = (2 * nn + p.nmu) * 64 * D;
        if (p.nmu == 4) hipLaunchKernelGGL((k_ms_chain_lane<4, CACHE>), g, b, lds, st, p);
        else if (p.nmu == 5) hipLaunchKernelGGL((k_ms_chain_lane<5, CACHE>), g, b, lds, st, p);
        else hipLaunchKernelGGL((k_ms_chain_lane<6, CACHE>), g, b, lds, st, p);
    } else if (k == MsChain::wavefront) {
        const size_t lds = (12 * nn + 6 * kMsMaxMu + 2) * D;
        if (p.nmu == 5) hipLaunchKernelGGL((k_ms_chain<5, CACHE>), g, b, lds, st, p);
        else if (p.nmu == 8) hipLaunchKernelGGL((k_ms_chain<8, CACHE>), g, b, lds, st, p);
        else hipLaunchKernelGGL((k_ms_chain<0, CACHE>), g, b, lds, st, p);
    } else {
        // matrix-core products (v_mfma_f64_16x16x4_f64), 4 LDS matrices with leading dimension 17; one block per (wavenumber,
        // g) works through the Fourier orders and stops at the reference's convergence break (writes rad itself).  Two builds,
        // both capped for three waves per SIMD.  <false> (default): phase matrices read from HBM / L2 in every layer, 9.3 KB
        // of LDS -- twelve blocks per CU; 65 registers spilled, reloaded in the layer set-up.  <true> (p.phase_lds,
        // ANSFM_MS_PHASE_LDS=1): the phase matrices of the Fourier order in LDS, 17.5 KB -- nine blocks per CU, no spills, a
        // quarter of the vector-memory instructions; 2-4 % slower at C4.
        const int ncu = p.ncont + (p.iray > 0 ? 1 : 0);
        const size_t lds = (4 * 16 * 17 + 5 * 16 + (p.phase_lds ? (size_t)ncu * 2 * 256 : 0)) * D;
        if constexpr (CACHE == 0) {
            if (p.phase_lds) hipLaunchKernelGGL((k_ms_chain16<true, 0>), g, b, lds, st, p);
            else hipLaunchKernelGGL((k_ms_chain16<false, 0>), g, b, lds, st, p);
        } else hipLaunchKernelGGL((k_ms_chain16<false, CACHE>), g, b, lds, st, p);
    }
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}
extern "C" {

// whatever way a scheduling function is left -- an error return of any launch included -- the main stream waits for the two
// side streams, so that the next entry point cannot reuse ctx->misc / tmp_* while a side stream still reads or writes them
struct MsRejoin {
    ansfm_ctx *c; int e1, e2, e3 = -1; bool done = false;      // e3 >= 0: ms_stream3 too
    void now()
    {
        if (done) return;
        done = true;
        if (hipEventRecord(c->ms_ev[e1], c->ms_stream) == hipSuccess) (void)hipStreamWaitEvent(c->stream, c->ms_ev[e1], 0);
        if (hipEventRecord(c->ms_ev[e2], c->ms_stream2) == hipSuccess) (void)hipStreamWaitEvent(c->stream, c->ms_ev[e2], 0);
        if (e3 >= 0 && hipEventRecord(c->ms_ev[e3], c->ms_stream3) == hipSuccess) (void)hipStreamWaitEvent(c->stream, c->ms_ev[e3], 0);
    }
    ~MsRejoin() { now(); }
};
static int ms_side_streams(ansfm_ctx *ctx, int nev)
{
    if (!ctx->ms_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->ms_stream, hipStreamNonBlocking));
    if (!ctx->ms_stream2) HIPCHK(hipStreamCreateWithFlags(&ctx->ms_stream2, hipStreamNonBlocking));
    while ((int)ctx->ms_ev.size() < nev) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->ms_ev.push_back(e);
    }
    return ANSFM_OK;
}

// The kernels of scloud11wave_core for one model on device-resident inputs: p from ms_setup with its nine input pointers set.
// Leaves rad[ngeom][ng][nwave] in ctx->tmp_out (asynchronous).  reuse_walk: the phase matrices and Hansen factors the previous
// call left in ctx->misc stand (the models of a batch one by one share the phase functions, and the walk is sequential and, at
// few streams, most of a call) -- not with several windows: ctx->misc holds the last two only.
static int ms_single(ansfm_ctx *ctx, MsParams &p, const MsRoute &r, const MsKnobs &kn, bool reuse_walk)
{
    const size_t D = sizeof(double), nn = (size_t)p.nmu * p.nmu;
    const int nwave = p.nwave, ng = p.ng, nf = p.nf;
    HIPCHK(ctx->tmp_in2.reserve((size_t)nwave * ng * (nf + 1) * p.ngeom * D));
    HIPCHK(ctx->tmp_out.reserve((size_t)p.ngeom * ng * nwave * D));
    p.drad = ctx->tmp_in2.as<double>();
    p.rad = ctx->tmp_out.as<double>();
    // G = 1: the phase matrices and Hansen factors of a window of wavenumbers at a time (ms_window_size)
    const long nwin = (ng == 1) ? ms_window_size(nwave, nf, p.ncomp, p.nmu, kn) : nwave;
    const bool windowed = nwin < nwave;
    ctx->ms_windows = (nwave + nwin - 1) / nwin; ctx->ms_window_w = nwin;
    const bool reuse = reuse_walk && !windowed;
    // three windows in rotation and the carry of the walk between them, or the whole axis
    const size_t nph = (size_t)nwave * (nf + 1) * p.ncomp * nn, nfc = (size_t)ng * nwave * p.ncomp * nn;
    const size_t nph_w = (size_t)nwin * (nf + 1) * p.ncomp * nn, nfc_w = (size_t)nwin * p.ncomp * nn;
    const size_t per_buf = 2 * nph_w + nfc_w;
    const size_t misc_n = windowed ? 3 * per_buf + (size_t)p.ncomp * nn : 2 * nph + nfc;
    HIPCHK(ctx->misc.reserve(misc_n * D));
    if (!reuse) HIPCHK(hipMemsetAsync(ctx->misc.p, 0, misc_n * D, ctx->stream));
    p.ppl = ctx->misc.as<double>(); p.pmi = p.ppl + nph; p.fc = p.pmi + nph;
    if (r.ncomp_run > 0 && !reuse && !windowed) {
        ms_launch_phase(ctx->stream, p);
        HIPCHK(hipGetLastError());
    }
    // window k of a windowed call: buffer k % 3, chains over [pw0, pw0 + wc) read taus / omegas / bnu relative to w0
    auto window_params = [&](int k) {
        MsParams pw = p;
        const int b = k % 3;
        pw.pw0 = (int)(k * nwin); pw.nwin = (int)std::min<long>(nwin, nwave - (long)k * nwin);
        pw.ppl = ctx->misc.as<double>() + b * per_buf; pw.pmi = pw.ppl + nph_w; pw.fc = pw.pmi + nph_w;
        pw.carry = ctx->misc.as<double>() + 3 * per_buf; pw.carry_in = k > 0 ? 1 : 0;
        pw.w0 = pw.pw0; pw.wcount = pw.nwin;
        pw.taus = p.taus + (size_t)pw.pw0 * ng * p.nlay; pw.omegas = p.omegas + (size_t)pw.pw0 * ng * p.nlay;
        pw.bnu = p.bnu + (size_t)pw.pw0 * p.nlay;
        return pw;
    };
    // G = 1, several windows, three stages in flight: window k's chains (main stream or beside it, alternating as the
    // g-ordinates of per_g_ordinate), window k + 1's walk (side stream) and window k + 2's phase matrices (third stream).  The
    // walk never queues behind phase matrices: those share the chip with the chains and take about as long.  Events, buffer
    // b = k % 3: ev[b] walked, ev[3 + b] chains done (window k + 3's phase matrices overwrite the buffer only then),
    // ev[6 + b] phase matrices done; ev[9] inputs ready; ev[10 .. 12] rejoin.
    auto by_window = [&]() -> int {
        int rc = ms_side_streams(ctx, 13);
        if (rc) return rc;
        if (!ctx->ms_stream3) HIPCHK(hipStreamCreateWithFlags(&ctx->ms_stream3, hipStreamNonBlocking));
        HIPCHK(hipEventRecord(ctx->ms_ev[9], ctx->stream));
        HIPCHK(hipStreamWaitEvent(ctx->ms_stream, ctx->ms_ev[9], 0));
        HIPCHK(hipStreamWaitEvent(ctx->ms_stream2, ctx->ms_ev[9], 0));
        HIPCHK(hipStreamWaitEvent(ctx->ms_stream3, ctx->ms_ev[9], 0));
        MsRejoin rejoin{ctx, 10, 11, 12};
        const int nw = (int)ctx->ms_windows;
        auto phase = [&](int k) -> int {
            const int b = k % 3;
            if (k >= 3) HIPCHK(hipStreamWaitEvent(ctx->ms_stream3, ctx->ms_ev[3 + b], 0));
            if (r.ncomp_run > 0) ms_launch_phase(ctx->ms_stream3, window_params(k));
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ctx->ms_ev[6 + b], ctx->ms_stream3));
            return ANSFM_OK;
        };
        auto walk = [&](int k) -> int {
            const int b = k % 3;
            HIPCHK(hipStreamWaitEvent(ctx->ms_stream, ctx->ms_ev[6 + b], 0));
            if (r.ncomp_run > 0) ms_launch_hansen(ctx->ms_stream, window_params(k));
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ctx->ms_ev[b], ctx->ms_stream));
            return ANSFM_OK;
        };
        if ((rc = phase(0)) || (nw > 1 && (rc = phase(1))) || (rc = walk(0))) return rc;
        for (int k = 0; k < nw; ++k) {
            if (k + 1 < nw && (rc = walk(k + 1))) return rc;
            if (k + 2 < nw && (rc = phase(k + 2))) return rc;
            hipStream_t cs = (k & 1) ? ctx->ms_stream2 : ctx->stream;
            HIPCHK(hipStreamWaitEvent(cs, ctx->ms_ev[k % 3], 0));
            if ((rc = ms_launch_chain<0>(ctx, r.chain, cs, window_params(k)))) return rc;
            HIPCHK(hipEventRecord(ctx->ms_ev[3 + k % 3], cs));
        }
        rejoin.now();
        return ANSFM_OK;
    };
    // The Hansen walk is sequential over (g, wave) -- two waves on the whole chip -- so it is cut into one launch per
    // g-ordinate on a second stream and the chains of g start as soon as its factors exist: the walk of g + 1 hides behind
    // them (it was 11-18 % of a call at 16 streams when it ran ahead of all chains).
    auto per_g_ordinate = [&]() -> int {
        int rc = ms_side_streams(ctx, ng + 3);
        if (rc) return rc;
        HIPCHK(hipEventRecord(ctx->ms_ev[ng], ctx->stream));                    // phase matrices (and every input) ready
        HIPCHK(hipStreamWaitEvent(ctx->ms_stream, ctx->ms_ev[ng], 0));
        HIPCHK(hipStreamWaitEvent(ctx->ms_stream2, ctx->ms_ev[ng], 0));
        // from here on work is queued on the side streams: the main stream waits for them however this function is left
        MsRejoin rejoin{ctx, ng + 1, ng + 2};
        for (int g = 0; g < ng; ++g) {
            MsParams ph = p;
            ph.ig0 = g; ph.ng_launch = 1;
            ms_launch_hansen(ctx->ms_stream, ph);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ctx->ms_ev[g], ctx->ms_stream));
        }
        for (int g = 0; g < ng; ++g) {
            MsParams pc = p;
            pc.ig0 = g; pc.ng_launch = 1;
            // even g on the main stream, odd g beside it (a third stream adds nothing): a launch of 1e4 blocks ends with a
            // tail of half-empty CUs (chains differ in length with the optical depth), which the next g-ordinate's blocks fill
            hipStream_t cs = (g & 1) ? ctx->ms_stream2 : ctx->stream;
            HIPCHK(hipStreamWaitEvent(cs, ctx->ms_ev[g], 0));
            if ((rc = ms_launch_chain<0>(ctx, r.chain, cs, pc))) return rc;
        }
        // the side streams must not run into the next call's buffers: they rejoin the main one here
        rejoin.now();
        return ANSFM_OK;
    };
    const int ncu = r.ncomp_run;
    p.phase_lds = (r.chain == MsChain::mfma16 && kn.phase_lds && ncu >= 1 && ncu <= 2) ? 1 : 0;
    int rc;
    if (windowed) rc = by_window();
    else if (r.ncomp_run > 0 && !reuse) rc = per_g_ordinate();
    else rc = ms_launch_chain<0>(ctx, r.chain, ctx->stream, p);      // reuse, or no scattering component: one launch
    if (rc) return rc;
    if (r.chain != MsChain::mfma16) {
        // every Fourier order was worked through: the sum with the reference's convergence break
        hipLaunchKernelGGL(k_ms_fourier, dim3(nblk((size_t)nwave * ng * p.ngeom, 128)), dim3(128), 0, ctx->stream, p);
        HIPCHK(hipGetLastError());
    }
    return ANSFM_OK;
}

// the g-quadrature (:4504) of the spectra of n_models models, rad [model][ngeom][G][W] in ctx->tmp_out, copied back to SPECOUT
// (and SPEC_G of a single model); fourier: k_ms_fourier first, model by model, from the orders the batch's chains left in drad
static int ms_gquad(ansfm_ctx *ctx, int n_models, int ngeom, const double *xf, double *SPECOUT, double *SPEC_G,
                    const MsParams *fourier)
{
    const int W = ctx->W, G = ctx->G;
    const size_t D = sizeof(double), nspec = (size_t)W * ngeom, st_rad = nspec * G;
    HIPCHK(ctx->tmp_out2.reserve(nspec * (n_models + (n_models == 1 ? (size_t)G : 0)) * D));   // one model: SPEC_G behind
    double *d_spec = ctx->tmp_out2.as<double>(), *d_specg = SPEC_G ? d_spec + nspec : nullptr;
    for (int m = 0; m < n_models; ++m) {
        if (fourier) {
            MsParams pf = *fourier;
            pf.drad += (size_t)m * pf.st_drad; pf.rad += (size_t)m * st_rad;
            hipLaunchKernelGGL(k_ms_fourier, dim3(nblk(st_rad, 128)), dim3(128), 0, ctx->stream, pf);
        }
        hipLaunchKernelGGL(k_ms_gquad, dim3(nblk(nspec, 128)), dim3(128), 0, ctx->stream, ctx->tmp_out.as<double>() + m * st_rad,
                           ctx->d_delg.as<double>(), xf, d_spec + m * nspec, d_specg, W, G, ngeom);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(SPECOUT, d_spec, (size_t)n_models * nspec * D, hipMemcpyDeviceToHost, ctx->stream));
    if (SPEC_G) HIPCHK(hipMemcpyAsync(SPEC_G, d_specg, nspec * G * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_scloud11wave_core(ansfm_ctx *ctx, int ncont, int nwave, int nth, const double *phasarr, const double *radg,
                            int ngeom, const double *sol_angs, const double *emiss_angs, const double *solar,
                            const double *aphis, int lowbc, const double *brdf_matrix, int nmu, const double *mu1,
                            const double *wt1, int nf, const double *bnu, int ng, int nlay, const double *taus,
                            const double *tauray, const double *omegas_s, int nphi, int iray, int imie,
                            const double *lfrac, double *rad)
{
    CHECK_CTX(ctx);
    if (ncont < 0 || nwave <= 0 || ngeom <= 0 || nmu < 2 || nf < 0 || ng <= 0 || nlay <= 0 || nphi <= 0 || !radg ||
        !sol_angs || !emiss_angs || !solar || !aphis || !brdf_matrix || !mu1 || !wt1 || !bnu || !taus || !tauray ||
        !omegas_s || !rad || (ncont > 0 && (!phasarr || !lfrac || nth < 3)))
        FAIL(ANSFM_ERR_INVALID, "scloud11wave_core: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const MsKnobs kn;
    MsCall c{};
    c.ncont = ncont; c.nth = nth; c.ngeom = ngeom; c.sol_angs = sol_angs; c.emiss_angs = emiss_angs; c.aphis = aphis;
    c.lowbc = lowbc; c.nmu = nmu; c.mu1 = mu1; c.wt1 = wt1; c.nf = nf; c.nphi = nphi; c.iray = iray; c.imie = imie;
    MsParams p;
    MsRoute r;
    int rc = ms_setup(ctx, p, c, nwave, ng, nlay, kn, r);
    if (rc) return rc;
    const size_t nw = nwave;
    Stager st{ctx};
    p.phasarr = st.up(phasarr, (size_t)ncont * nw * 2 * nth); p.radg = st.up(radg, nw * nmu); p.solar = st.up(solar, nw);
    p.brdf = st.up(brdf_matrix, nw * nmu * nmu * (nf + 1)); p.bnu = st.up(bnu, nw * nlay); p.taus = st.up(taus, nw * ng * nlay);
    p.tauray = st.up(tauray, nw * nlay); p.omegas = st.up(omegas_s, nw * ng * nlay); p.lfrac = st.up(lfrac, nw * ncont * nlay);
    if ((rc = st.rc)) return rc;
    if (p.nmu_real && (rc = ms_pad_inputs(ctx, nmu, nw, nw, nf, &p.radg, &p.brdf))) return rc;
    if ((rc = ms_single(ctx, p, r, kn, false))) return rc;
    HIPCHK(hipMemcpyAsync(rad, ctx->tmp_out.p, (size_t)ngeom * ng * nwave * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

// The host arrays of a scattering call on the device (null: not given).  The continuum of one model is [W][L] / [W][ncont][L], of
// a batch [n][W][L] / [n][W][ncont][L] or, by rows, [R][W] / [R][ncont][W] with d_crow [n][L].
struct MsStaged {
    const double *press, *temp, *am, *cia, *dust, *ray, *sca, *phas, *lf, *rg, *sol, *brdf, *xf;
    const int32_t *d_crow;
};

// Reads c's host pointers; leaves their device copies in s (staging slots 0 .. 13, copies queued on ctx->stream).  CN: elements
// of one continuum array (lfrac: CN * ncont); 0: the continuum and cont_row stay null (they are on the device already).
static int ms_stage(ansfm_ctx *ctx, const MsCall &c, size_t CN, MsStaged &s)
{
    const size_t W = ctx->W, nl = (size_t)c.n_models * c.L;
    Stager st{ctx};
    s.press = st.up(c.lay_press_pa, nl); s.temp = st.up(c.lay_temp, nl); s.am = st.up(c.amount, nl * ctx->S);
    s.cia = st.up(c.taucia, CN); s.dust = st.up(c.taudust, CN); s.ray = st.up(c.tauray, CN); s.sca = st.up(c.tauscat, CN);
    s.phas = st.up(c.phasarr, (size_t)c.ncont * c.W_full * 2 * c.nth); s.lf = st.up(c.lfrac, CN * c.ncont);
    s.rg = st.up(c.radg, c.n_models * W * c.nmu); s.sol = st.up(c.solar, W);
    s.brdf = st.up(c.brdf_matrix, W * c.nmu * c.nmu * (c.nf + 1)); s.xf = st.up(c.xfac, W);
    s.d_crow = st.up(c.cont_row, CN ? nl : 0);
    if (st.rc == ANSFM_OK && c.theta_deg && c.ncont > 0) {       // phasarr stays in HBM
        HIPCHK(ctx->ms_phas_src.reserve((size_t)c.ncont * W * 2 * c.nth * sizeof(double)));
        s.phas = ctx->ms_phas_src.as<double>();
        return launch_phase_source(ctx, c.nth, c.theta_deg, c.mu_theta, 0, ctx->ms_phas_src.as<double>());
    }
    return st.rc;
}

// The per-layer arrays of a fused continuum (c.fused) on the device, staging slots 14 .. 19, as the continuum kernels take them
// (stage_cont); d_temp: the staged layer temperatures [n][L].  An array whose term is not used stays null.
static int ms_stage_cont(ansfm_ctx *ctx, const MsCall &c, const double *d_temp, ContCall &k)
{
    Stager st{ctx, 14};
    k = stage_cont(st, c.cont, (size_t)c.n_models * c.L, d_temp);
    return st.rc;
}

// The optics stage's parameters from the staged inputs and the context's buffers (reserve ms_taus / ms_omegas / ms_bnu and, by
// rows, ms_tauray_l / ms_lfrac_l first).  slot: the gas row of every (model, layer), null for one model.  The launch fills in
// the slab and the models.
static MsOpticsParams ms_optics_params(ansfm_ctx *ctx, const MsCall &c, const MsStaged &s, const int32_t *slot)
{
    MsOpticsParams o;
    memset(&o, 0, sizeof o);
    o.taugas = ctx->tau.as<double>(); o.slot = slot; o.cont_row = s.d_crow;
    o.taucia = s.cia; o.taudust = s.dust; o.tauray = s.ray; o.tauscat = s.sca; o.lfrac = s.lf;
    o.wave = ctx->d_wave.as<double>(); o.lay_temp = s.temp;
    o.taus = ctx->ms_taus.as<double>(); o.omegas = ctx->ms_omegas.as<double>(); o.bnu = ctx->ms_bnu.as<double>();
    o.tauray_l = ctx->ms_tauray_l.as<double>(); o.lfrac_l = ctx->ms_lfrac_l.as<double>();
    o.W = ctx->W; o.Wpad = ctx->Wpad; o.G = ctx->G; o.L = c.L; o.ncont = s.lf ? c.ncont : 0; o.ispace = c.ISPACE;
    return o;
}

// TAUTOT, OMEGA, BB (by rows: and the slab's TAURAY / fractions) of the models [m0, m0 + nm) of the launch order ids (null:
// position = model) on the wavenumbers [w0, w0 + wc)
static void ms_launch_optics(hipStream_t st, MsOpticsParams &o, int w0, int wc, int m0, int nm, const int *ids)
{
    o.w0 = w0; o.wcount = wc; o.m0 = m0; o.nm = nm; o.model_ids = ids;
    const dim3 grid(nblk((size_t)wc, 128), (unsigned)o.L, (unsigned)nm);
    if (o.cont_row) hipLaunchKernelGGL(k_ms_optics<true>, grid, dim3(128), 0, st, o);
    else hipLaunchKernelGGL(k_ms_optics<false>, grid, dim3(128), 0, st, o);
}

// one model; reuse_walk: ms_single's; dc: its continuum on the device instead of c's host arrays
static int cirsrad_ck_scatter_impl(ansfm_ctx *ctx, const MsCall &c, const MsKnobs &kn, bool reuse_walk, const MsDevCont *dc = nullptr)
{
    int rc = ms_check(ctx, c, "cirsrad_ck_scatter");
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, G = ctx->G, L = c.L;
    MsParams p;
    MsRoute r;
    if ((rc = ms_setup(ctx, p, c, W, G, L, kn, r))) return rc;
    const size_t D = sizeof(double), WL = (size_t)W * L;
    MsStaged s;
    if ((rc = ms_stage(ctx, c, dc ? 0 : WL, s))) return rc;
    if (dc) { s.cia = dc->cia; s.dust = dc->dust; s.ray = dc->ray; s.sca = dc->sca; s.lf = dc->lf; }
    // ---- vertical gas opacities: calc_k + k_overlap (:3855-3874), as in the thermal branch --------------------------
    HIPCHK(ctx->ms_taus.reserve(WL * G * D));
    HIPCHK(ctx->ms_omegas.reserve(WL * G * D));
    HIPCHK(ctx->ms_bnu.reserve(WL * D));
    const double *d_tauray = s.ray;
    if ((rc = ms_zero_tauray(ctx, WL, &d_tauray)) || (rc = gas_opacity(ctx, L, s.press, s.temp, s.am))) return rc;
    ctx->last_n = 1; ctx->last_L = L; ctx->last_rows = L; ctx->last_dedup = 0;
    // ---- TAUTOT, OMEGA, BB -----------------------------------------------------------------------------------------
    MsOpticsParams o = ms_optics_params(ctx, c, s, nullptr);
    ms_launch_optics(ctx->stream, o, 0, W, 0, 1, nullptr);
    HIPCHK(hipGetLastError());
    // ---- doubling / adding, g-quadrature ------------------------------------------------------------------------------
    p.phasarr = s.phas; p.radg = s.rg; p.solar = s.sol;
    p.brdf = s.brdf; p.bnu = o.bnu; p.taus = o.taus; p.tauray = d_tauray; p.omegas = o.omegas;
    p.lfrac = s.lf;
    if (p.nmu_real && (rc = ms_pad_inputs(ctx, c.nmu, (size_t)W, (size_t)W, c.nf, &p.radg, &p.brdf))) return rc;
    if ((rc = ms_single(ctx, p, r, kn, reuse_walk))) return rc;
    return ms_gquad(ctx, 1, c.ngeom, s.xf, c.SPECOUT, c.SPEC_G, nullptr);
}

int ansfm_cirsrad_ck_scatter(ansfm_ctx *ctx, int ISPACE, int L, const double *lay_press_pa, const double *lay_temp,
                             const double *amount, const double *taucia, const double *taudust, const double *tauray,
                             const double *tauscat, int ncont, int nth, const double *phasarr, const double *lfrac,
                             const double *radg, int ngeom, const double *sol_angs, const double *emiss_angs,
                             const double *aphis, const double *solar, int lowbc, const double *brdf_matrix, int nmu,
                             const double *mu1, const double *wt1, int nf, int nphi, int iray, int imie, const double *xfac,
                             double *SPECOUT, double *SPEC_G)
{
    CHECK_CTX(ctx);
    const MsCall c{ISPACE, 1, L, lay_press_pa, lay_temp, amount, taucia, taudust, tauray, tauscat, ncont, nth, phasarr, lfrac,
                   radg, ngeom, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, nmu, mu1, wt1, nf, nphi, iray, imie,
                   xfac, SPECOUT, SPEC_G, ctx->W, 0};
    return cirsrad_ck_scatter_impl(ctx, c, MsKnobs(), false);
}

/* ------------------------------------------------------------------------------------------ */
/* batched scattering branch: the forward models of a numerical Jacobian (jacobian_nemesis :2251-2252)   */
/* ------------------------------------------------------------------------------------------ */
// The stages of cirsrad_ck_scatter_batch_impl, in the order it calls them.

// Reads c.R and c.cont_row (host); launches nothing.  Dense calls pass.
static int ms_check_rows(ansfm_ctx *ctx, const MsCall &c)
{
    if (!c.cont_row) return ANSFM_OK;
    const int L = c.L;
    if (c.R <= 0) FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_scatter_batch_rows: R must be positive");
    for (size_t i = 0; i < (size_t)c.n_models * L; ++i)
        if (c.cont_row[i] < 0 || c.cont_row[i] >= c.R)
            FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_scatter_batch_rows: cont_row[" + std::to_string(i / L) + "][" + std::to_string(i % L) +
                                        "] = " + std::to_string(c.cont_row[i]) + " is outside [0, R = " + std::to_string(c.R) + ")");
    return ANSFM_OK;
}

// The whole call without the layer cache -- a single model, de-duplication switched off (ansfm_set_layer_dedup),
// ANSFM_MS_LAYER_CACHE=0 or a runtime line source: model by model through cirsrad_ck_scatter_impl; m > 0: same phase functions,
// quadrature, orders -- model 0's walk stands.  Reads c; leaves every model's SPECOUT and the last_* counters.
// By rows: the rows go up once, behind the staging slots of the single-model entry; a model's dense arrays are formed from them
// on the device, one model at a time in one buffer (ctx->ms_tauray_l).
static int ms_batch_by_model(ansfm_ctx *ctx, const MsCall &c, const MsKnobs &kn)
{
    const int W = ctx->W, S = ctx->S, L = c.L, n_models = c.n_models, ncont = c.ncont;
    const size_t D = sizeof(double), WL = (size_t)W * L;
    const bool fused = c.fused != 0, by_rows = c.cont_row != nullptr || fused;
    const size_t RW = c.cont_row ? (size_t)c.R * W : 0;
    int rc;
    HIPCHK(hipSetDevice(ctx->device));
    Stager sr{ctx, fused ? 20 : 14};
    const int32_t *d_crow = c.cont_row ? sr.up(c.cont_row, (size_t)n_models * L) : nullptr;
    const double *rsrc[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ContCall k;                                                 // fused: every model's per-layer arrays, staged once
    if (fused) {
        // a model's L rows are formed from the resident sources when its turn comes; its row map is the identity
        std::vector<int32_t> iota((size_t)L);
        for (int l = 0; l < L; ++l) iota[l] = l;
        d_crow = sr.up(iota.data(), (size_t)L);
        const double *d_temp = sr.up(c.lay_temp, (size_t)n_models * L);
        if ((rc = sr.rc) || (rc = ms_stage_cont(ctx, c, d_temp, k))) return rc;
        HIPCHK(hipStreamSynchronize(ctx->stream));              // iota is a host temporary
    } else if (by_rows) {
        rsrc[0] = sr.up(c.taucia, RW); rsrc[1] = sr.up(c.taudust, RW); rsrc[2] = sr.up(c.tauray, RW); rsrc[3] = sr.up(c.tauscat, RW);
        rsrc[4] = sr.up(c.lfrac, RW * ncont);
        if ((rc = sr.rc)) return rc;
    }
    if (by_rows) HIPCHK(ctx->ms_tauray_l.reserve((4 + (size_t)ncont) * WL * D));
    for (int m = 0; m < n_models; ++m) {
        const size_t mm = m;
        MsCall cm = c;
        cm.n_models = 1;
        // per-model phase functions: the model's variant; the walk of the model before stands only where it had the same one
        const int var = c.pv ? c.pv->phase_of[mm] : 0, var_before = (c.pv && m > 0) ? c.pv->phase_of[mm - 1] : 0;
        const bool reuse = m > 0 && var == var_before;
        if (var > 0) cm.phasarr = c.pv->phasarr.data() + (size_t)(var - 1) * c.ncont * W * 2 * c.nth;
        cm.pv = nullptr;
        cm.lay_press_pa += mm * L; cm.lay_temp += mm * L; cm.amount += mm * S * L;
        cm.radg += mm * W * c.nmu; cm.SPECOUT += mm * W * c.ngeom;
        if (ctx->lblrt) ctx->st_m0 = m;                      // gas_tau reads this model's rows of the state
        if (by_rows) {
            if (fused) {
                MsContRows rw;                                  // this model's layers
                if ((rc = launch_ms_cont_rows(ctx, L, nullptr, cont_of_model(ctx, k, mm, L), &rw))) return rc;
                rsrc[0] = rw.cia; rsrc[1] = rw.dust; rsrc[2] = rw.ray; rsrc[3] = rw.sca; rsrc[4] = rw.lf;
            }
            const double *dense[5];
            for (int a = 0; a < 5; ++a) {
                const int X = a < 4 ? 1 : ncont;
                double *dst = ctx->ms_tauray_l.as<double>() + (size_t)a * WL;
                dense[a] = (rsrc[a] && X > 0) ? dst : nullptr;
                if (dense[a])
                    hipLaunchKernelGGL(k_ms_rows_expand, dim3(nblk((size_t)W, 128), (unsigned)L, (unsigned)X), dim3(128), 0, ctx->stream,
                                       W, X, L, fused ? d_crow : d_crow + mm * L, rsrc[a], dst);
            }
            HIPCHK(hipGetLastError());
            const MsDevCont dc{dense[0], dense[1], dense[2], dense[3], dense[4]};
            rc = cirsrad_ck_scatter_impl(ctx, cm, kn, reuse, &dc);
        } else {
            for (const double **a : {&cm.taucia, &cm.taudust, &cm.tauray, &cm.tauscat}) if (*a) *a += mm * WL;
            if (cm.lfrac) cm.lfrac += mm * WL * ncont;
            rc = cirsrad_ck_scatter_impl(ctx, cm, kn, reuse);
        }
        ctx->st_m0 = -1;
        if (rc) return rc;
    }
    ctx->last_n = n_models; ctx->last_L = L; ctx->last_rows = n_models * L; ctx->last_dedup = 0;
    return ANSFM_OK;
}

// Which layers equal model 0's in EVERY input, and where a model's adding sweep may start.  Reads ctx->dd_slot (dedup_rows), the
// staged continuum or cont_row, d_pvar [n] / d_diff [V][ncomp] (per-model phase functions; null: none) and c.radg on the host.
// Leaves same[n][L] in ctx->ms_same (*same), the sweep starts [n] and the launch order [n] in ctx->ms_lstart and *ids_out, the
// ms_cache_* counters and *npre, the prefix stacks per model; synchronises the stream.
static int ms_same_layers(ansfm_ctx *ctx, const MsCall &c, const MsKnobs &kn, const MsStaged &s, bool lookup, const int *d_pvar,
                          const unsigned char *d_diff, unsigned char **same_out, int *npre_out, std::vector<int> *ids_out)
{
    const int W = ctx->W, L = c.L, n_models = c.n_models, ncont = c.ncont;
    const size_t nl = (size_t)n_models * L;
    const bool by_rows = s.d_crow != nullptr;
    HIPCHK(ctx->ms_same.reserve(nl));
    unsigned char *same = *same_out = ctx->ms_same.as<unsigned char>();
    // by rows: from the two index maps alone; dense: the gas rows, then the columns of every continuum array
    hipLaunchKernelGGL(k_ms_same_index, dim3(nblk(nl, 128)), dim3(128), 0, ctx->stream, n_models, L, ctx->dd_slot.as<int32_t>(), s.d_crow,
                       same);
    for (const double *col : {s.cia, s.dust, s.ray, s.sca})
        if (col && !by_rows)
            hipLaunchKernelGGL(k_ms_same_cols, dim3(nblk((size_t)(n_models - 1) * W, 128)), dim3(128), 0, ctx->stream, n_models, W,
                               1, L, col, same);
    if (s.lf && ncont > 0 && !by_rows)
        hipLaunchKernelGGL(k_ms_same_cols, dim3(nblk((size_t)(n_models - 1) * W * ncont, 128)), dim3(128), 0, ctx->stream,
                           n_models, W, ncont, L, s.lf, same);
    // per-model phase functions: a layer that scatters through a population whose phase function changed is the model's own
    if (d_pvar && s.lf && ncont > 0)
        hipLaunchKernelGGL(k_ms_same_phase, dim3(nblk((size_t)(n_models - 1) * W * ncont, 128)), dim3(128), 0, ctx->stream, n_models, W,
                           ncont, L, d_pvar, d_diff, s.lf, s.d_crow, same);
    HIPCHK(hipGetLastError());
    // where a model's adding sweep may start: below its first changed layer (in sweep order: bottom first when the paths look
    // down, top first when they look up) the stack equals model 0's, kept after every kMsPrefixStep-th layer
    const int npre = *npre_out = L / kMsPrefixStep;
    std::vector<unsigned char> hs(nl);
    HIPCHK(hipMemcpyAsync(hs.data(), same, nl, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    long hits = 0;
    for (size_t k = (size_t)L; k < nl; ++k) hits += hs[k];
    ctx->ms_cache_hits = hits; ctx->ms_cache_layers = (long)(n_models - 1) * L;
    std::vector<int> lstart((size_t)n_models, 0);
    for (int m = 1; m < n_models && kn.prefix; ++m) {
        int lf = 0;
        while (lf < L && hs[(size_t)m * L + (lookup ? L - 1 - lf : lf)]) ++lf;
        // the lower boundary sits at the bottom of a look-down stack: its radiance must be model 0's too
        if (c.lowbc > 0 && !lookup &&
            memcmp(c.radg + (size_t)m * W * c.nmu, c.radg, (size_t)W * c.nmu * sizeof(double)) != 0)
            lf = 0;
        lstart[m] = std::min(lf / kMsPrefixStep, npre) * kMsPrefixStep;
    }
    // launch order of models 1 .. n-1: by sweep start, so that the blocks of one launch read the same layers of the cache at
    // about the same time (position 0 of the list is unused: model 0 has its own launch)
    std::vector<int> ids((size_t)n_models, 0);
    for (int m = 0; m < n_models; ++m) ids[m] = m;
    // (per-model phase functions: by variant first -- a launch of the cached chains covers one variant, ms_run_slabs)
    auto var_of = [&](int m) { return c.pv ? c.pv->phase_of[(size_t)m] : 0; };
    std::stable_sort(ids.begin() + 1, ids.end(), [&](int a, int b) {
        return var_of(a) != var_of(b) ? var_of(a) < var_of(b) : lstart[a] < lstart[b];
    });
    *ids_out = ids;
    HIPCHK(ctx->ms_lstart.reserve((size_t)2 * n_models * sizeof(int)));
    HIPCHK(hipMemcpyAsync(ctx->ms_lstart.p, lstart.data(), (size_t)n_models * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->ms_lstart.as<int>() + n_models, ids.data(), (size_t)n_models * sizeof(int), hipMemcpyHostToDevice,
                          ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

// Per-model phase functions: the plan (which components differ, the pairs of the two launches, the layout), the variants'
// phasarr and the small tables on the device.  Reads c.pv (validated) and c.phasarr on the host and p's sizes; leaves vp, p.pairs /
// npairs / phasarr_var / st_phas / vstride, *d_pvar [n] (the models' variants), *d_diff [V][ncomp] and the ms_var_* counters;
// synchronises the stream.
// ANSFM_ERR_UNSUPPORTED when the variants' phase functions find no room.
static int ms_stage_variants(ansfm_ctx *ctx, const MsCall &c, MsVariantPlan &vp, MsParams &p, const int **d_pvar, const unsigned char **d_diff)
{
    const MsVariantSet &pv = *c.pv;
    const size_t D = sizeof(double), I = sizeof(int);
    vp = ms_variants_plan(pv.V, c.ncont, c.iray, (size_t)ctx->W, c.nth, c.nf, p.nmu, ctx->G, c.phasarr, pv.phasarr.data());
    if (ctx->ms_var_in.reserve(pv.phasarr.size() * D) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsrad_ck_scatter_batch: no memory for the phase functions of " + std::to_string(pv.V) + " variants");
    }
    const size_t n_int = (size_t)2 * vp.npairs + c.n_models;
    HIPCHK(ctx->ms_var_tab.reserve(n_int * I + vp.diff.size()));
    char *tab = ctx->ms_var_tab.as<char>();
    HIPCHK(hipMemcpyAsync(ctx->ms_var_in.p, pv.phasarr.data(), pv.phasarr.size() * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(tab, vp.pairs.data(), (size_t)2 * vp.npairs * I, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(tab + (size_t)2 * vp.npairs * I, pv.phase_of.data(), (size_t)c.n_models * I, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(tab + n_int * I, vp.diff.data(), vp.diff.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));                  // vp's vectors may move
    p.pairs = reinterpret_cast<const int *>(tab); p.npairs = vp.npairs; *d_pvar = p.pairs + 2 * vp.npairs;
    p.phasarr_var = ctx->ms_var_in.as<double>(); p.st_phas = vp.st_phas; p.vstride = vp.vstride;
    *d_diff = reinterpret_cast<const unsigned char *>(tab + n_int * I);
    ctx->ms_var_pairs = vp.npairs - vp.npairs0; ctx->ms_var_bytes = (long)vp.bytes_variants();
    return ANSFM_OK;
}

// G > 1: the phase matrices of the whole axis and the whole walk in one launch, ahead of the slabs -- they do not depend on the
// model.  The walk continues from g to g + 1 over the whole axis, so a slice walks all of it too: its factors kept, the rest of
// the steps into a sink.  Reads p (sizes, phasarr); leaves ctx->misc zeroed and filled, p.ppl / p.pmi at the slice's first
// wavenumber and p.fc.
// vp (per-model phase functions; p.pairs / phasarr_var set by ms_stage_variants): the buffers of every variant, one behind the
// other; the pairs that differ from variant 0 join variant 0's components in the two launches, the rest is copied from variant 0.
static int ms_walk_axis(ansfm_ctx *ctx, const MsCall &c, const MsRoute &r, const MsVariantPlan *vp, MsParams &p)
{
    const int W = ctx->W, G = ctx->G;
    const bool sliced = c.W_full != W;
    const size_t D = sizeof(double), nn = (size_t)p.nmu * p.nmu;
    const size_t per_w = (size_t)(c.nf + 1) * p.ncomp * nn, nph = (size_t)c.W_full * per_w, nfc = (size_t)G * W * p.ncomp * nn;
    const size_t misc_0 = 2 * nph + nfc + (sliced ? (size_t)p.ncomp * nn : 0), misc_n = vp ? vp->total : misc_0;
    if (vp && (vp->nph != nph || vp->nfc != nfc || sliced)) FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_scatter_batch: the phase variants' plan does not fit the call");
    if (vp && ctx->misc.reserve(misc_n * D) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsrad_ck_scatter_batch: no memory for the phase matrices and Hansen factors of " +
                                        std::to_string(vp->V) + " phase-function variants (" + std::to_string(misc_n * D) + " bytes)");
    }
    HIPCHK(ctx->misc.reserve(misc_n * D));
    HIPCHK(hipMemsetAsync(ctx->misc.p, 0, misc_0 * D, ctx->stream));          // (a variant is written whole: its pairs, then the copy)
    p.ppl = ctx->misc.as<double>(); p.pmi = p.ppl + nph; p.fc = p.pmi + nph;
    for (hipEvent_t &e : ctx->ms_walk_ev) if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(ctx->ms_walk_ev[0], ctx->stream));
    if (r.ncomp_run > 0) {
        MsParams pw = p;
        pw.nwave = c.W_full; pw.nwin = c.W_full;
        ms_launch_phase(ctx->stream, pw);
        if (sliced) { pw.st0 = c.w_begin; pw.stn = W; pw.sink = p.fc + nfc; }
        ms_launch_hansen(ctx->stream, pw);
        HIPCHK(hipGetLastError());
    }
    if (vp && vp->V > 1) {
        hipLaunchKernelGGL(k_ms_variant_fill, dim3(nblk(vp->vstride, 256)), dim3(256), 0, ctx->stream, vp->V, vp->ncomp, (int)nn, vp->vstride,
                           ctx->ms_var_tab.as<unsigned char>() + ((size_t)2 * vp->npairs + c.n_models) * sizeof(int), p.ppl);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ctx->ms_walk_ev[1], ctx->stream));
    ctx->ms_walk_timed = true;
    p.ppl += (size_t)c.w_begin * per_w; p.pmi += (size_t)c.w_begin * per_w;
    return ANSFM_OK;
}

// The slabs of the spectral axis: Ws wavenumbers each, in units of `unit`, with per_unit bytes of layer cache and per_unit_pre
// of prefix stacks per unit; at most mchunk models per launch of the cached chains.
struct MsSlabs { long unit, Ws; size_t per_unit, per_unit_pre; int mchunk; };

// Slabs sized by the layer cache.  16 streams: the cache per wavenumber, and prefix stacks beside it.  Fewer: no prefix stacks
// (the adding sweep is a few per cent of a chain there), the cache per tile of 64 wavenumbers (the lane kernel's; the wavefront
// kernel keeps the layout).  Reads the free device memory and the ANSFM_MS_SLAB / CHUNK / WINDOW switches; leaves sl and
// ctx->ms_windows / ms_window_w.  G = 1: the slabs are the windows of phase matrices and Hansen factors (ms_window_size): a
// slab's phase matrices and walk -- continuing from the carry of the slab before -- go in front of its chains, model 0's first;
// this reserves and zeroes one window in ctx->misc, sets p.ppl / pmi / fc / carry and, for a slice, walks the wavenumbers in front
// of it.
static int ms_plan_slabs(ansfm_ctx *ctx, const MsCall &c, const MsKnobs &kn, const MsRoute &r, int npre, MsParams &p, MsSlabs &sl)
{
    const int W = ctx->W, G = ctx->G, L = c.L, nmu = c.nmu, nf = c.nf, ncomp = p.ncomp;
    const size_t D = sizeof(double), nn = (size_t)p.nmu * p.nmu;
    const bool m16 = r.chain == MsChain::mfma16, win = G == 1;
    const long unit = sl.unit = m16 ? 1 : 64;
    const size_t entry = m16 ? (size_t)kMsCacheEntry : (2 * (size_t)nmu * nmu + nmu) * 64;  // doubles per (unit, g, order, layer)
    sl.per_unit = (size_t)G * (nf + 1) * L * entry * D;
    sl.per_unit_pre = m16 ? (size_t)G * (nf + 1) * npre * entry * D : 0;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    free_b += ctx->ms_cache.bytes + (m16 ? ctx->ms_pcache.bytes : 0);
    const size_t budget = std::min<size_t>(free_b / 2, (size_t)96 << 30);
    long units = (long)(budget / (sl.per_unit + sl.per_unit_pre));
    if (kn.slab) units = std::min(units, (kn.slab + unit - 1) / unit);
    if (units < 1)
        FAIL(ANSFM_ERR_HIP, m16 ? "cirsrad_ck_scatter_batch: no memory for the layer cache of one wavenumber"
                                : "cirsrad_ck_scatter_batch: no memory for the layer cache of one tile of wavenumbers");
    const long Ws = sl.Ws = std::min(std::min<long>(W, units * unit), win ? ms_window_size(c.W_full, nf, ncomp, p.nmu, kn) : (long)W);
    ctx->ms_windows = (W + Ws - 1) / Ws; ctx->ms_window_w = Ws;
    if (win) {
        const size_t nph_w = (size_t)Ws * (nf + 1) * ncomp * nn, n_all = 2 * nph_w + (size_t)Ws * ncomp * nn + ncomp * nn;
        HIPCHK(ctx->misc.reserve(n_all * D));
        HIPCHK(hipMemsetAsync(ctx->misc.p, 0, n_all * D, ctx->stream));
        p.ppl = ctx->misc.as<double>(); p.pmi = p.ppl + nph_w; p.fc = p.pmi + nph_w; p.carry = p.fc + (size_t)Ws * ncomp * nn;
        // a slice: the walk of the wavenumbers in front of it, in windows of Ws whose factors only feed the carry
        for (long a = 0; a < c.w_begin && r.ncomp_run > 0; a += Ws) {
            MsParams pw = p;
            pw.nwave = c.W_full; pw.pw0 = (int)a; pw.nwin = (int)std::min<long>(Ws, c.w_begin - a); pw.carry_in = a > 0 ? 1 : 0;
            pw.ig0 = 0; pw.ng_launch = 1;
            ms_launch_phase(ctx->stream, pw);
            ms_launch_hansen(ctx->stream, pw);
            HIPCHK(hipGetLastError());
        }
    }
    sl.mchunk = std::min(c.n_models - 1, kn.chunk ? kn.chunk : 64);
    return ANSFM_OK;
}

// Reserves the layer cache, the prefix stacks, the optics outputs of one launch (by rows: and its TAURAY / fractions), the
// orders and the radiances, and points p at them and at same / the sweep starts / the launch order.  Leaves p ready for the
// slab loop but for the slab and the models of a launch.
static int ms_wire_batch(ansfm_ctx *ctx, const MsCall &c, const MsStaged &s, const MsRoute &r, unsigned char *same, int npre,
                         const MsSlabs &sl, MsParams &p)
{
    const int W = ctx->W, G = ctx->G, L = c.L, n_models = c.n_models, ncont = c.ncont, nf = c.nf, ngeom = c.ngeom;
    const size_t D = sizeof(double), Ws = (size_t)sl.Ws;
    const bool m16 = r.chain == MsChain::mfma16;
    HIPCHK(ctx->ms_cache.reserve((size_t)((sl.Ws + sl.unit - 1) / sl.unit) * sl.per_unit));
    if (m16) {
        HIPCHK(ctx->ms_pcache.reserve(std::max<size_t>(Ws * sl.per_unit_pre, 8)));
        HIPCHK(ctx->ms_orders.reserve(Ws * G * sizeof(int)));
    }
    const size_t opt_models = (size_t)std::max(1, sl.mchunk);
    HIPCHK(ctx->ms_taus.reserve(opt_models * Ws * G * L * D));
    HIPCHK(ctx->ms_omegas.reserve(opt_models * Ws * G * L * D));
    HIPCHK(ctx->ms_bnu.reserve(opt_models * Ws * L * D));
    if (s.d_crow) {
        HIPCHK(ctx->ms_tauray_l.reserve(opt_models * Ws * L * D));
        HIPCHK(ctx->ms_lfrac_l.reserve(std::max<size_t>(opt_models * Ws * ncont * L * D, 8)));
        p.tauray = ctx->ms_tauray_l.as<double>(); p.lfrac = ctx->ms_lfrac_l.as<double>(); p.cont_local = 1;
    }
    if (!m16) {                                                 // the orders, for k_ms_fourier
        p.st_drad = (size_t)W * G * (nf + 1) * ngeom;
        HIPCHK(ctx->tmp_in2.reserve((size_t)n_models * p.st_drad * D));
        p.drad = ctx->tmp_in2.as<double>();
    }
    HIPCHK(ctx->tmp_out.reserve((size_t)n_models * ngeom * G * W * D));
    p.rad = ctx->tmp_out.as<double>();
    p.taus = ctx->ms_taus.as<double>(); p.omegas = ctx->ms_omegas.as<double>(); p.bnu = ctx->ms_bnu.as<double>();
    p.cache = ctx->ms_cache.as<double>(); p.same = same;
    if (m16) {
        p.cache_orders = ctx->ms_orders.as<int>(); p.pcache = ctx->ms_pcache.as<double>(); p.lstart = ctx->ms_lstart.as<int>(); p.npre = npre;
    }
    p.model_ids = ctx->ms_lstart.as<int>() + n_models;
    p.st_wl = s.ray ? (size_t)W * L : 0; p.st_wcl = (size_t)W * ncont * L; p.st_wm = (size_t)W * p.nmu; p.st_rad = (size_t)ngeom * G * W;
    p.ig0 = 0; p.ng_launch = G;
    return ANSFM_OK;
}

// Slab by slab (G = 1: its phase matrices and walk first): the optics and the ordinary chain of model 0, which also fills the
// cache, then models 1 .. n-1 in chunks: the adding sweep over cached layers, changed layers computed in place.  Leaves
// rad [model][ngeom][G][W] in ctx->tmp_out or, below 16 streams, every order in ctx->tmp_in2.
// Per-model phase functions: ids is sorted by variant, a launch ends where the variant changes and reads that variant's phase
// matrices and factors -- the chain kernels are the ones every other batch runs.
static int ms_run_slabs(ansfm_ctx *ctx, const MsCall &c, const MsStaged &s, const MsRoute &r, const MsSlabs &sl, const std::vector<int> &ids,
                        MsParams &p)
{
    const int W = ctx->W, L = c.L, n_models = c.n_models, w_begin = c.w_begin;
    int rc;
    MsOpticsParams o = ms_optics_params(ctx, c, s, ctx->dd_slot.as<int32_t>());
    for (long w0 = 0; w0 < W; w0 += sl.Ws) {
        const int wc = (int)std::min<long>(sl.Ws, W - w0);
        if (ctx->G == 1) {
            // the phase matrices of the slab are those of the wavenumbers w_begin + [w0, w0 + wc) of phasarr; chains and walk
            // index the window relative to w0
            p.pw0 = (int)w0; p.nwin = wc; p.carry_in = w_begin + w0 > 0 ? 1 : 0;
            p.ig0 = 0; p.ng_launch = 1;
            if (r.ncomp_run > 0) {
                MsParams pw = p;
                pw.nwave = c.W_full; pw.pw0 = w_begin + (int)w0;
                ms_launch_phase(ctx->stream, pw);
                ms_launch_hansen(ctx->stream, p);
            }
            HIPCHK(hipGetLastError());
        }
        p.w0 = (int)w0; p.wcount = wc;
        if (s.d_crow) { p.st_wl = (size_t)wc * L; p.st_wcl = (size_t)wc * c.ncont * L; }       // between launch positions
        ms_launch_optics(ctx->stream, o, (int)w0, wc, 0, 1, nullptr);
        p.m0 = 0; p.n_launch = 1;
        if ((rc = ms_launch_chain<1>(ctx, r.chain, ctx->stream, p))) return rc;
        for (int m0 = 1, nm; m0 < n_models; m0 += nm) {
            nm = std::min(sl.mchunk, n_models - m0);
            MsParams pl = p;
            if (c.pv) {
                const int v = c.pv->phase_of[(size_t)ids[m0]];
                int k = 1;
                while (k < nm && c.pv->phase_of[(size_t)ids[m0 + k]] == v) ++k;
                nm = k;
                const size_t vo = (size_t)v * p.vstride;
                pl.ppl += vo; pl.pmi += vo; pl.fc += vo;
            }
            ms_launch_optics(ctx->stream, o, (int)w0, wc, m0, nm, p.model_ids);
            pl.m0 = m0; pl.n_launch = nm;
            if ((rc = ms_launch_chain<2>(ctx, r.chain, ctx->stream, pl))) return rc;
        }
    }
    return ANSFM_OK;
}

static int cirsrad_ck_scatter_batch_impl(ansfm_ctx *ctx, const MsCall &c, const MsKnobs &kn)
{
    int rc = ms_check(ctx, c, "cirsrad_ck_scatter_batch");
    if (rc || (rc = ms_check_rows(ctx, c))) return rc;           // before anything is launched
    const int W = ctx->W, G = ctx->G, L = c.L, n_models = c.n_models;
    const bool by_rows = c.cont_row != nullptr || c.fused;
    ctx->ms_cache_hits = 0; ctx->ms_cache_layers = (long)n_models * L;
    ctx->ms_var_pairs = 0; ctx->ms_var_bytes = 0; ctx->ms_walk_timed = false;
    if (c.pv) {                                                  // per-model phase functions: refusals before anything is launched
        const std::string fn = "cirsrad_ck_scatter_batch: the pending phase variants (ansfm_set_phase_variants) ";
        if (c.W_full != W) FAIL(ANSFM_ERR_UNSUPPORTED, fn + "meet a slice of the spectral axis");
        if (G == 1) FAIL(ANSFM_ERR_UNSUPPORTED, fn + "meet a table of one g-ordinate (the windowed walk)");
        std::string why;
        if (ms_variants_validate(*c.pv, n_models, c.ncont, c.nth, &why)) FAIL(ANSFM_ERR_INVALID, fn + "do not fit the call: " + why);
        if (c.pv->phasarr.size() != (size_t)(c.pv->V - 1) * c.ncont * W * 2 * c.nth)
            FAIL(ANSFM_ERR_INVALID, fn + "were set on a table of another width");
    }
    // (a runtime line source has its own row map, which the (p, T, amount) comparison of the layer cache does not see)
    const bool use_cache = n_models > 1 && ctx->dedup && kn.layer_cache && !ctx->lblrt;      // any stream count
    if (!use_cache && c.W_full != W)
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsrad_ck_scatter_batch_slice: a slice needs the layer cache (n_models > 1, layer de-duplication on)");
    if (!use_cache) return ms_batch_by_model(ctx, c, kn);
    HIPCHK(hipSetDevice(ctx->device));
    MsParams p;
    MsRoute r;
    if ((rc = ms_setup(ctx, p, c, W, G, L, kn, r))) return rc;
    MsStaged s;
    if ((rc = ms_stage(ctx, c, c.fused ? 0 : by_rows ? (size_t)c.R * W : (size_t)n_models * W * L, s))) return rc;
    ContCall fc;                                                // fused: the per-layer arrays behind the continuum
    if (c.fused && (rc = ms_stage_cont(ctx, c, s.temp, fc))) return rc;
    const double *d_tauray = s.ray;                             // no TAURAY: every model reads the same zeros
    if (!by_rows && (rc = ms_zero_tauray(ctx, (size_t)W * L, &d_tauray))) return rc;     // (by rows: the optics stage writes the slab's copy)
    // vertical gas opacities of the distinct (model, layer) rows: calc_k + k_overlap
    DedupRows k;
    if (c.fused) {
        // one map for both: a layer is distinct when it differs from model 0's in a gas input or in a column the continuum is
        // formed from; the continuum of the distinct rows comes from the resident sources and the row map is the gas rows'
        MsContRows rw;
        if ((rc = dedup_rows_cont(ctx, n_models, L, s.press, s.temp, s.am, fc, false, &k)) ||
            (rc = launch_ms_cont_rows(ctx, k.rows, ctx->dd_work.as<int32_t>(), fc, &rw)))
            return rc;
        s.cia = rw.cia; s.dust = rw.dust; s.ray = rw.ray; s.sca = rw.sca; s.lf = rw.lf;
        s.d_crow = ctx->dd_slot.as<int32_t>();
    } else if ((rc = dedup_rows(ctx, n_models, L, s.press, s.temp, s.am, nullptr, &k)))
        return rc;
    if ((rc = gas_opacity(ctx, k.rows, k.press, k.temp, k.amount))) return rc;
    ctx->last_n = n_models; ctx->last_L = L; ctx->last_rows = k.rows; ctx->last_dedup = 1;
    MsVariantPlan vp;
    const unsigned char *d_diff = nullptr;
    const int *d_pvar = nullptr;
    if (c.pv && (rc = ms_stage_variants(ctx, c, vp, p, &d_pvar, &d_diff))) return rc;
    unsigned char *same;
    int npre;
    std::vector<int> ids;                                       // the launch order of models 1 .. n-1
    if ((rc = ms_same_layers(ctx, c, kn, s, p.lookup, d_pvar, d_diff, &same, &npre, &ids))) return rc;
    p.phasarr = s.phas; p.radg = s.rg; p.solar = s.sol;
    p.brdf = s.brdf; p.tauray = d_tauray; p.lfrac = s.lf;
    if (p.nmu_real && (rc = ms_pad_inputs(ctx, c.nmu, (size_t)n_models * W, (size_t)W, c.nf, &p.radg, &p.brdf))) return rc;
    if (G > 1 && (rc = ms_walk_axis(ctx, c, r, c.pv ? &vp : nullptr, p))) return rc;
    MsSlabs sl;
    if ((rc = ms_plan_slabs(ctx, c, kn, r, npre, p, sl)) || (rc = ms_wire_batch(ctx, c, s, r, same, npre, sl, p)) ||
        (rc = ms_run_slabs(ctx, c, s, r, sl, ids, p)))
        return rc;
    // below 16 streams every Fourier order was worked through: k_ms_fourier applies the reference's convergence break per model
    return ms_gquad(ctx, n_models, c.ngeom, s.xf, c.SPECOUT, nullptr, r.chain == MsChain::mfma16 ? nullptr : &p);
}

int ansfm_cirsrad_ck_scatter_batch(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                   const double *lay_temp, const double *amount, const double *taucia, const double *taudust,
                                   const double *tauray, const double *tauscat, int ncont, int nth, const double *phasarr,
                                   const double *lfrac, const double *radg, int ngeom, const double *sol_angs,
                                   const double *emiss_angs, const double *aphis, const double *solar, int lowbc,
                                   const double *brdf_matrix, int nmu, const double *mu1, const double *wt1, int nf, int nphi,
                                   int iray, int imie, const double *xfac, double *SPECOUT)
{
    CHECK_CTX(ctx);
    const MsVariantSet pv = ms_take_variants(ctx);
    MsCall c{ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucia, taudust, tauray, tauscat, ncont, nth, phasarr,
             lfrac, radg, ngeom, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, nmu, mu1, wt1, nf, nphi, iray,
             imie, xfac, SPECOUT, nullptr, ctx->W, 0};
    c.pv = pv.armed() ? &pv : nullptr;
    return cirsrad_ck_scatter_batch_impl(ctx, c, MsKnobs());
}

int ansfm_cirsrad_ck_scatter_batch_slice(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                         const double *lay_temp, const double *amount, const double *taucia, const double *taudust,
                                         const double *tauray, const double *tauscat, int ncont, int nth, const double *phasarr,
                                         const double *lfrac, const double *radg, int ngeom, const double *sol_angs,
                                         const double *emiss_angs, const double *aphis, const double *solar, int lowbc,
                                         const double *brdf_matrix, int nmu, const double *mu1, const double *wt1, int nf, int nphi,
                                         int iray, int imie, const double *xfac, double *SPECOUT, int W_full, int w_begin)
{
    CHECK_CTX(ctx);
    const MsVariantSet pv = ms_take_variants(ctx);              // (refused below unless the slice is the whole axis)
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsrad_ck_scatter_batch_slice: upload a k-table first");
    if (w_begin < 0 || (long)w_begin + ctx->W > (long)W_full || (ncont > 0 && !phasarr))
        FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_scatter_batch_slice: the table is not a slice [w_begin, w_begin + W) of W_full, or no phasarr");
    MsCall c{ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucia, taudust, tauray, tauscat, ncont, nth, phasarr,
             lfrac, radg, ngeom, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, nmu, mu1, wt1, nf, nphi, iray,
             imie, xfac, SPECOUT, nullptr, W_full, w_begin};
    c.pv = pv.armed() ? &pv : nullptr;
    return cirsrad_ck_scatter_batch_impl(ctx, c, MsKnobs());
}

int ansfm_cirsrad_ck_scatter_batch_rows(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                        const double *lay_temp, const double *amount, int R, const int32_t *cont_row,
                                        const double *taucia_rows, const double *taudust_rows, const double *tauray_rows,
                                        const double *tauscat_rows, int ncont, int nth, const double *phasarr,
                                        const double *lfrac_rows, const double *radg, int ngeom, const double *sol_angs,
                                        const double *emiss_angs, const double *aphis, const double *solar, int lowbc,
                                        const double *brdf_matrix, int nmu, const double *mu1, const double *wt1, int nf, int nphi,
                                        int iray, int imie, const double *xfac, double *SPECOUT, int W_full, int w_begin)
{
    CHECK_CTX(ctx);
    const MsVariantSet pv = ms_take_variants(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsrad_ck_scatter_batch_rows: upload a k-table first");
    if (!cont_row || w_begin < 0 || (long)w_begin + ctx->W > (long)W_full || (ncont > 0 && !phasarr))
        FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_scatter_batch_rows: no cont_row, the table is not a slice [w_begin, w_begin + W) of W_full, or no phasarr");
    MsCall c{ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucia_rows, taudust_rows, tauray_rows, tauscat_rows, ncont,
             nth, phasarr, lfrac_rows, radg, ngeom, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, nmu, mu1, wt1, nf,
             nphi, iray, imie, xfac, SPECOUT, nullptr, W_full, w_begin, R, cont_row};
    c.pv = pv.armed() ? &pv : nullptr;
    return cirsrad_ck_scatter_batch_impl(ctx, c, MsKnobs());
}

int ansfm_cirsrad_ck_scatter_batch_cont(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                        const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                        const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                        const double *lay_cont, int ray_mode, const double *f4, int ncont, int nth,
                                        const double *phasarr, const double *radg, int ngeom, const double *sol_angs,
                                        const double *emiss_angs, const double *aphis, const double *solar, int lowbc,
                                        const double *brdf_matrix, int nmu, const double *mu1, const double *wt1, int nf, int nphi,
                                        int iray, int imie, const double *xfac, double *SPECOUT, int W_full, int w_begin)
{
    CHECK_CTX(ctx);
    const std::string fn = "cirsrad_ck_scatter_batch_cont: ";
    if (ms_take_variants(ctx).armed())
        FAIL(ANSFM_ERR_UNSUPPORTED, fn + "pending phase variants (ansfm_set_phase_variants): the resident aerosol source has no model axis");
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, fn + "upload a k-table first");
    if (w_begin < 0 || (long)w_begin + ctx->W > (long)W_full || (ncont > 0 && !phasarr))
        FAIL(ANSFM_ERR_INVALID, fn + "the table is not a slice [w_begin, w_begin + W) of W_full, or no phasarr");
    MsCall c{ISPACE, n_models, L, lay_press_pa, lay_temp, amount, nullptr, nullptr, nullptr, nullptr, ncont, nth, phasarr, nullptr,
             radg, ngeom, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, nmu, mu1, wt1, nf, nphi, iray, imie, xfac, SPECOUT,
             nullptr, W_full, w_begin, 0, nullptr, 1};
    const int rc = fused_cont_check(ctx, fn, ISPACE, lay_temp, use_cia, lay_q, lay_frac, lay_totam, lay_delh, use_dust, lay_cont, ray_mode,
                                    f4, ContNeed::any_term, &c.cont);
    if (rc) return rc;
    if (ncont != (use_dust ? ctx->dust_n : 0))
        FAIL(ANSFM_ERR_INVALID, fn + "ncont = " + std::to_string(ncont) + " phase functions, the aerosol source has " +
                                    std::to_string(use_dust ? ctx->dust_n : 0) + " populations");
    return cirsrad_ck_scatter_batch_impl(ctx, c, MsKnobs());
}

int ansfm_cirsrad_ck_scatter_batch_src(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                       const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                       const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                       const double *lay_cont, int ray_mode, const double *f4, int ncont, int nth,
                                       const double *theta_deg, const double *mu_theta, const double *radg, int ngeom,
                                       const double *sol_angs, const double *emiss_angs, const double *aphis, const double *solar,
                                       int lowbc, const double *brdf_matrix, int nmu, const double *mu1, const double *wt1, int nf,
                                       int nphi, int iray, int imie, const double *xfac, double *SPECOUT, int W_full, int w_begin)
{
    CHECK_CTX(ctx);
    const std::string fn = "cirsrad_ck_scatter_batch_src: ";
    if (ms_take_variants(ctx).armed())
        FAIL(ANSFM_ERR_UNSUPPORTED, fn + "pending phase variants (ansfm_set_phase_variants): the resident aerosol source has no model axis");
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, fn + "upload a k-table first");
    if (W_full != ctx->W || w_begin != 0)
        FAIL(ANSFM_ERR_UNSUPPORTED, fn + "the whole axis only (a slice's context does not hold the grid the source lives on)");
    if (!theta_deg || !mu_theta || nth < 3) FAIL(ANSFM_ERR_INVALID, fn + "bad argument (theta_deg, mu_theta [nth], nth >= 3)");
    MsCall c{ISPACE, n_models, L, lay_press_pa, lay_temp, amount, nullptr, nullptr, nullptr, nullptr, ncont, nth, nullptr, nullptr,
             radg, ngeom, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, nmu, mu1, wt1, nf, nphi, iray, imie, xfac, SPECOUT,
             nullptr, W_full, w_begin, 0, nullptr, 1};
    int rc = fused_cont_check(ctx, fn, ISPACE, lay_temp, use_cia, lay_q, lay_frac, lay_totam, lay_delh, use_dust, lay_cont, ray_mode, f4,
                              ContNeed::aerosols, &c.cont);
    if (rc) return rc;
    if (ncont != ctx->dust_n)
        FAIL(ANSFM_ERR_INVALID, fn + "ncont = " + std::to_string(ncont) + " phase functions, the aerosol source has " +
                                    std::to_string(ctx->dust_n) + " populations");
    if ((rc = phase_source_check(ctx, fn, ncont)) || (rc = phase_source_angles(ctx, fn, nth, theta_deg))) return rc;
    if ((imie == 0) != (ctx->phase_imie == 0))
        FAIL(ANSFM_ERR_INVALID, fn + "imie = " + std::to_string(imie) + ", the phase-function source was uploaded with imie = " +
                                    std::to_string(ctx->phase_imie));
    for (int t = 1; t < nth; ++t)
        if (!(theta_deg[t] > theta_deg[t - 1])) FAIL(ANSFM_ERR_INVALID, fn + "theta_deg (Scatter.THETA) must be strictly ascending");
    c.theta_deg = theta_deg; c.mu_theta = mu_theta;
    return cirsrad_ck_scatter_batch_impl(ctx, c, MsKnobs());
}

int ansfm_set_phase_variants(ansfm_ctx *ctx, int n_models, int V, const int32_t *phase_of, int ncont, int nth,
                             const double *phasarr_variants)
{
    CHECK_CTX(ctx);
    ctx->ms_pv = MsVariantSet();
    if (V <= 1 || !phase_of || !phasarr_variants) return ANSFM_OK;
    if (!ctx->have_table || n_models <= 0 || ncont <= 0 || nth < 3)
        FAIL(ANSFM_ERR_INVALID, "set_phase_variants: upload a table first; n_models > 0, ncont > 0, nth >= 3");
    MsVariantSet s;
    s.n_models = n_models; s.V = V; s.ncont = ncont; s.nth = nth;
    s.phase_of.assign(phase_of, phase_of + n_models);
    s.phasarr.assign(phasarr_variants, phasarr_variants + (size_t)(V - 1) * ncont * ctx->W * 2 * nth);
    ctx->ms_pv = std::move(s);
    return ANSFM_OK;
}

int ansfm_last_scatter_variants(const ansfm_ctx *cctx, int64_t *pairs, int64_t *bytes, double *walk_ms)
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);
    CHECK_CTX(ctx);
    if (pairs) *pairs = ctx->ms_var_pairs;
    if (bytes) *bytes = ctx->ms_var_bytes;
    if (walk_ms) {
        *walk_ms = -1.0;
        if (ctx->ms_walk_timed) {
            float t = 0.f;
            HIPCHK(hipSetDevice(ctx->device));
            HIPCHK(hipEventSynchronize(ctx->ms_walk_ev[1]));
            HIPCHK(hipEventElapsedTime(&t, ctx->ms_walk_ev[0], ctx->ms_walk_ev[1]));
            *walk_ms = t;
        }
    }
    return ANSFM_OK;
}

int ansfm_last_scatter_cache(const ansfm_ctx *ctx, int64_t *layers_from_cache, int64_t *layers_total)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (layers_from_cache) *layers_from_cache = ctx->ms_cache_hits;
    if (layers_total) *layers_total = ctx->ms_cache_layers;
    return ANSFM_OK;
}

int ansfm_last_scatter_windows(const ansfm_ctx *ctx, int64_t *windows, int64_t *window_wavenumbers)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (windows) *windows = ctx->ms_windows;
    if (window_wavenumbers) *window_wavenumbers = ctx->ms_window_w;
    return ANSFM_OK;
}

}  // extern "C"
