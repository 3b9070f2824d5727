// ansfm_ops.hip -- entry points of libansfm.so around the radiative transfer: gradient maps, ILS convolution, the continua
// (CIA, Rayleigh, dust), layering and the k-distribution of a line-by-line spectrum.  gfx950 only.
#include "ansfm_map_kernels.hip.h"
#include "ansfm_conv_kernels.hip.h"
#include "ansfm_cont_kernels.hip.h"
#include "ansfm_layer_kernels.hip.h"
#include "ansfm_kdist.hip.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

void ansfm::launch_tau_rayleigh_rows(ansfm_ctx *ctx, int rows, int ray_mode, int ISPACE, const int32_t *slot_rows,
                                     const double *ray_totam, const double *ray_f4)
{
    hipLaunchKernelGGL(k_tau_rayleigh_rows, dim3(nblk((size_t)rows * ctx->Wpad, 256)), dim3(256), 0, ctx->stream, rows, ctx->W, ctx->Wpad,
                       ray_mode, ISPACE, ctx->d_wave.as<double>(), slot_rows, ray_totam, ray_f4, ctx->cont_t.as<double>());
}

int ansfm::fused_cont_check(ansfm_ctx *ctx, const std::string &fn, int ISPACE, const double *lay_temp, int use_cia,
                            const double *lay_q, const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                            const double *lay_cont, int ray_mode, const double *f4, ContNeed need, ContCall *out)
{
    if ((ray_mode != 0 && ray_mode != 1 && ray_mode != 2 && ray_mode != 4 && ray_mode != 12) || (ray_mode == 4 && !f4) ||
        ((use_cia || ray_mode) && !lay_totam) || (use_cia && (!lay_q || !lay_frac || !lay_delh)) || (use_dust && !lay_cont))
        FAIL(ANSFM_ERR_INVALID, fn + "bad argument (ray_mode = IRAY 0, 1, 2, 4 or 12, f4 with IRAY 4; the per-layer arrays of every "
                                     "term that is used)");
    if (need == ContNeed::any_term && !use_cia && !use_dust && !ray_mode)
        FAIL(ANSFM_ERR_INVALID, fn + "bad argument (at least one of use_cia, use_dust, ray_mode)");
    if (need == ContNeed::scatterer && !use_dust && !ray_mode)
        FAIL(ANSFM_ERR_INVALID, fn + "neither aerosols nor Rayleigh scattering: no scattering opacity");
    if (need == ContNeed::aerosols && !use_dust)
        FAIL(ANSFM_ERR_INVALID, fn + "bad argument (use_dust: the phase functions are those of the aerosol populations)");
    if (use_cia && !ctx->cia_on) FAIL(ANSFM_ERR_INVALID, fn + "no CIA source on this table's grid (ansfm_upload_cia after the table)");
    if (use_cia && ctx->cia_ispace != ISPACE) FAIL(ANSFM_ERR_INVALID, fn + "the CIA source was uploaded for the other ISPACE");
    if (use_dust && !ctx->dust_n) FAIL(ANSFM_ERR_INVALID, fn + "no aerosol source on this table's grid (ansfm_upload_dust after the table)");
    ContCall &c = *out;
    c.ISPACE = ISPACE; c.use_cia = use_cia ? 1 : 0; c.use_dust = use_dust ? 1 : 0; c.ray_mode = ray_mode;
    c.temp = lay_temp;
    c.q = use_cia ? lay_q : nullptr; c.frac = use_cia ? lay_frac : nullptr; c.delh = use_cia ? lay_delh : nullptr;
    c.totam = (use_cia || ray_mode) ? lay_totam : nullptr;
    c.cont = use_dust ? lay_cont : nullptr;
    c.f4 = ray_mode == 4 ? f4 : nullptr;
    return ANSFM_OK;
}

// The arguments of k_cia_rows_prep / k_tau_cont_rows / k_dtau_cont_rows for `rows` rows of the call c, from the context's
// resident sources; reserves the rows' CIA records
static int cont_rows_params(ansfm_ctx *ctx, int rows, const int32_t *slot_rows, const ContCall &c, ContRowsParams &p)
{
    const int W = ctx->W, Wpad = ctx->Wpad;
    memset(&p, 0, sizeof p);
    p.wave = ctx->d_wave.as<double>(); p.work = slot_rows;
    p.rows = rows; p.W = W; p.Wpad = Wpad; p.ispace = c.ISPACE; p.ray_mode = c.ray_mode;
    p.totam = c.totam; p.f4 = c.f4;
    if (c.use_dust) { p.kext_w = ctx->dust_kext.as<double>(); p.cont = c.cont; p.NDUST = ctx->dust_n; }
    if (c.use_cia) {
        HIPCHK(ctx->cia_lay.reserve((size_t)rows * sizeof(CiaLayer)));
        const size_t nK = (size_t)ctx->cia_NPAIR * ctx->cia_NPE * ctx->cia_NT * ctx->cia_NWC;
        const double *t = ctx->cia_tab.as<double>();
        CiaParams &k = p.cia;
        k.cia_waven = t; k.K = t + ctx->cia_NWC; p.cia_temp = k.K + nK; p.cia_frac = p.cia_temp + ctx->cia_NT;
        k.k_co2 = p.cia_frac + ctx->cia_nfrac; k.k_n2n2 = k.k_co2 + W; k.k_n2h2 = k.k_n2n2 + W;
        k.g1 = ctx->cia_idx.as<int32_t>(); k.g2 = k.g1 + ctx->cia_NPAIR;
        k.q = c.q;
        k.W = W; k.NWC = ctx->cia_NWC; k.NPAIR = ctx->cia_NPAIR; k.NPE = ctx->cia_NPE; k.NT = ctx->cia_NT; k.NVMR = ctx->cia_NVMR;
        k.covers = ctx->cia_covers; k.ico2 = ctx->cia_ico2; k.in2 = ctx->cia_in2; k.ih2 = ctx->cia_ih2;
        p.use_cia = 1; p.nfrac = ctx->cia_nfrac; p.NPARA = ctx->cia_NPARA;
        p.temp = c.temp; p.frac = c.frac; p.delh = c.delh;
        p.lay = ctx->cia_lay.as<CiaLayer>();
        k.lay = p.lay;
    }
    return ANSFM_OK;
}

int ansfm::launch_tau_cont_rows(ansfm_ctx *ctx, int rows, const int32_t *slot_rows, const ContCall &c)
{
    HIPCHK(ctx->cont_t.reserve((size_t)rows * ctx->Wpad * sizeof(double)));
    ContRowsParams p;
    int rc;
    if ((rc = cont_rows_params(ctx, rows, slot_rows, c, p))) return rc;
    p.out = ctx->cont_t.as<double>();
    if (c.use_cia) {
        hipLaunchKernelGGL(k_cia_rows_prep, dim3(nblk((size_t)rows, 64)), dim3(64), 0, ctx->stream, p);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tau_cont_rows, dim3((unsigned)rows, nblk((size_t)ctx->Wpad, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

int ansfm::launch_ms_cont_rows(ansfm_ctx *ctx, int rows, const int32_t *slot_rows, const ContCall &c, MsContRows *out)
{
    const size_t RW = (size_t)rows * ctx->W, nd = c.use_dust ? (size_t)ctx->dust_n : 0;
    HIPCHK(ctx->ms_cont_rows.reserve((4 + nd) * RW * sizeof(double)));
    MsContRowsParams p;
    int rc;
    if ((rc = cont_rows_params(ctx, rows, slot_rows, c, p.c))) return rc;
    double *b = ctx->ms_cont_rows.as<double>();
    p.ksca_w = ctx->dust_ksca.as<double>();
    p.taucia = c.use_cia ? b : nullptr; p.taudust = c.use_dust ? b + RW : nullptr; p.tauray = c.ray_mode ? b + 2 * RW : nullptr;
    p.tauscat = c.use_dust ? b + 3 * RW : nullptr; p.lfrac = c.use_dust ? b + 4 * RW : nullptr;
    if (c.use_cia) {
        hipLaunchKernelGGL(k_cia_rows_prep, dim3(nblk((size_t)rows, 64)), dim3(64), 0, ctx->stream, p.c);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ms_cont_rows, dim3((unsigned)rows, nblk((size_t)ctx->W, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    *out = MsContRows{p.taucia, p.taudust, p.tauray, p.tauscat, p.lfrac};
    return ANSFM_OK;
}

int ansfm::launch_ss_cont_rows(ansfm_ctx *ctx, int rows, const int32_t *slot_rows, const ContCall &c, int P, const double *phase_fn,
                               SsContRows *out)
{
    const size_t RW = (size_t)rows * ctx->Wpad;
    HIPCHK(ctx->cont_t.reserve(RW * sizeof(double)));
    HIPCHK(ctx->ss_cont_rows.reserve((1 + (size_t)P) * RW * sizeof(double)));
    SsContRowsParams p;
    int rc;
    if ((rc = cont_rows_params(ctx, rows, slot_rows, c, p.c))) return rc;
    p.c.out = ctx->cont_t.as<double>();
    p.ksca_w = ctx->dust_ksca.as<double>();
    p.phase_fn = phase_fn; p.P = P;
    p.sca = ctx->ss_cont_rows.as<double>(); p.phase = p.sca + RW;
    if (c.use_cia) {
        hipLaunchKernelGGL(k_cia_rows_prep, dim3(nblk((size_t)rows, 64)), dim3(64), 0, ctx->stream, p.c);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ss_cont_rows, dim3((unsigned)rows, nblk((size_t)ctx->Wpad, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    *out = SsContRows{p.c.out, p.sca, p.phase};
    return ANSFM_OK;
}

int ansfm::launch_dtau_cont_rows(ansfm_ctx *ctx, int n_models, int L, int NVMR, int NPAR, const ContCall &c)
{
    const int rows = n_models * L;
    if (NVMR + 2 > ANSFM_MAX_CONT_GRAD_SLOTS)
        FAIL(ANSFM_ERR_UNSUPPORTED, "the fused continuum gradients hold NVMR + 2 <= " + std::to_string(ANSFM_MAX_CONT_GRAD_SLOTS) +
                                        " slots per thread in LDS");
    HIPCHK(ctx->dcont_t.reserve((size_t)n_models * NPAR * L * ctx->Wpad * sizeof(double)));
    DContRowsParams p;
    int rc;
    if ((rc = cont_rows_params(ctx, rows, nullptr, c, p.c))) return rc;
    p.dout = ctx->dcont_t.as<double>();
    p.L = L; p.NVMR = NVMR; p.NPAR = NPAR;
    const size_t lds = c.use_cia ? (size_t)(NVMR + 2) * kDContBlock * sizeof(double) : 0;      // the slots of cia_sum
    hipLaunchKernelGGL(k_dtau_cont_rows, dim3((unsigned)rows, nblk((size_t)ctx->Wpad, kDContBlock)), dim3(kDContBlock), lds, ctx->stream, p);
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

extern "C" {

/* ------------------------------------------------------------------------------------------ */
/* gradient maps (ForwardModel_0.map2pro / map2xvec)                                           */
/* ------------------------------------------------------------------------------------------ */
static int launch_gemm(ansfm_ctx *ctx, GemmParams g, const std::vector<GemmBatch> &batch)
{
    if (batch.empty() || g.M <= 0 || g.N <= 0) return ANSFM_OK;
    HIPCHK(ctx->map_batch.reserve(batch.size() * sizeof(GemmBatch)));
    HIPCHK(hipMemcpyAsync(ctx->map_batch.p, batch.data(), batch.size() * sizeof(GemmBatch), hipMemcpyHostToDevice,
                          ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // batch is a host temporary
    g.batch = ctx->map_batch.as<GemmBatch>();
    hipLaunchKernelGGL(k_gemm_f64, dim3((unsigned)((g.M + 63) / 64), (unsigned)((g.N + 63) / 64), (unsigned)batch.size()),
                       dim3(256), 0, ctx->stream, g);
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

int ansfm_map2pro(ansfm_ctx *ctx, int W, int NPAR, int LIMAX, int P, int NPRO, int NLAY, int NVMR, int NDUST,
                  const double *dSPECIN, const int32_t *LAYINC, const double *DTE, const double *DAM,
                  const double *DCO, int n_incpar, const int32_t *INCPAR, double *dSPECOUT)
{
    CHECK_CTX(ctx);
    if (W <= 0 || NPAR <= 0 || LIMAX <= 0 || P <= 0 || NPRO <= 0 || NLAY <= 0 || NVMR < 0 || NDUST < 0 ||
        NPAR != NVMR + 2 + NDUST || !LAYINC || !DTE || !DAM || !DCO || n_incpar < 0 || (n_incpar > 0 && !INCPAR))
        FAIL(ANSFM_ERR_INVALID, "map2pro: bad argument (NPAR must be NVMR+2+NDUST)");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double);
    const size_t nin = (size_t)W * NPAR * LIMAX * P, nout = (size_t)W * NPAR * NPRO * P;
    const double *dA;
    if (dSPECIN) {
        HIPCHK(ctx->tmp_in.reserve(nin * D));
        HIPCHK(hipMemcpyAsync(ctx->tmp_in.p, dSPECIN, nin * D, hipMemcpyHostToDevice, ctx->stream));
        dA = ctx->tmp_in.as<double>();
    } else {
        if (ctx->dspec_dims[0] != W || ctx->dspec_dims[1] != NPAR || ctx->dspec_dims[2] != LIMAX || ctx->dspec_dims[3] != P)
            FAIL(ANSFM_ERR_INVALID, "map2pro: no device-resident cirsradg result of these dimensions");
        dA = ctx->dspec_ref.as<double>();
    }
    // M_cls[LAYINC[j][p]][pro] gathered on the host: Bx[cls][p][j][pro], cls 0 = DAM, 1 = DTE, 2 = DCO
    std::vector<double> bx((size_t)3 * P * LIMAX * NPRO);
    const double *Mc[3] = {DAM, DTE, DCO};
    for (int cls = 0; cls < 3; ++cls)
        for (int p = 0; p < P; ++p)
            for (int j = 0; j < LIMAX; ++j) {
                int lay = LAYINC[(size_t)j * P + p];
                if (lay < 0) lay += NLAY;                     // python negative index
                if (lay < 0 || lay >= NLAY) FAIL(ANSFM_ERR_INVALID, "map2pro: LAYINC entry outside the layer range");
                memcpy(&bx[(((size_t)cls * P + p) * LIMAX + j) * NPRO], Mc[cls] + (size_t)lay * NPRO, NPRO * D);
            }
    HIPCHK(ctx->map_b.reserve(bx.size() * D));
    HIPCHK(hipMemcpyAsync(ctx->map_b.p, bx.data(), bx.size() * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx->map_out.reserve(nout * D));
    ctx->map_dims[0] = 0;
    HIPCHK(hipMemsetAsync(ctx->map_out.p, 0, nout * D, ctx->stream));
    std::vector<GemmBatch> batch;
    long long last_a = -1, last_b = -1;                       // the reference's stale dSPECOUT1
    const int npm = n_incpar > 0 ? n_incpar : NPAR;
    for (int p = 0; p < P; ++p)
        for (int ip = 0; ip < npm; ++ip) {
            const int par = n_incpar > 0 ? INCPAR[ip] : ip;
            if (par < 0 || par >= NPAR) FAIL(ANSFM_ERR_INVALID, "map2pro: INCPAR entry outside 0..NPAR-1");
            int cls = -1;
            if (par <= NVMR - 1) cls = 0;
            else if (par <= NVMR) cls = 1;
            else if (par <= NVMR + NDUST) cls = 2;
            GemmBatch b;
            if (cls >= 0) {
                b.a_off = ((long long)par * LIMAX) * P + p;
                b.b_off = (((long long)cls * P + p) * LIMAX) * NPRO;
                last_a = b.a_off; last_b = b.b_off;
            } else {
                if (last_a < 0) FAIL(ANSFM_ERR_INVALID, "map2pro: para-H2 parameter listed first (the reference raises UnboundLocalError)");
                b.a_off = last_a; b.b_off = last_b;
            }
            b.c_off = ((long long)par * NPRO) * P + p;
            batch.push_back(b);
        }
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.A = dA; g.B = ctx->map_b.as<double>(); g.C = ctx->map_out.as<double>();
    g.M = W; g.N = NPRO; g.K = LIMAX;
    g.a_sm = (long long)NPAR * LIMAX * P; g.a_sk = P;
    g.b_sk = NPRO; g.b_sn = 1;
    g.c_sm = (long long)NPAR * NPRO * P; g.c_sn = P;
    int rc = launch_gemm(ctx, g, batch);
    if (rc) return rc;
    ctx->map_dims[0] = W; ctx->map_dims[1] = NPAR; ctx->map_dims[2] = NPRO; ctx->map_dims[3] = P;
    if (dSPECOUT) {
        HIPCHK(hipMemcpyAsync(dSPECOUT, ctx->map_out.p, nout * D, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return ANSFM_OK;
}

int ansfm_map2xvec(ansfm_ctx *ctx, int W, int NPAR, int NPRO, int P, int NX, const double *dSPECIN,
                   const double *xmap, double *dSPECOUT)
{
    CHECK_CTX(ctx);
    if (W <= 0 || NPAR <= 0 || NPRO <= 0 || P <= 0 || NX <= 0 || !xmap || !dSPECOUT)
        FAIL(ANSFM_ERR_INVALID, "map2xvec: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double);
    const size_t nin = (size_t)W * NPAR * NPRO * P, nout = (size_t)W * P * NX, nxm = (size_t)NX * NPAR * NPRO;
    const double *dA;
    if (dSPECIN) {
        HIPCHK(ctx->tmp_in.reserve(nin * D));
        HIPCHK(hipMemcpyAsync(ctx->tmp_in.p, dSPECIN, nin * D, hipMemcpyHostToDevice, ctx->stream));
        dA = ctx->tmp_in.as<double>();
    } else {
        if (ctx->map_dims[0] != W || ctx->map_dims[1] != NPAR || ctx->map_dims[2] != NPRO || ctx->map_dims[3] != P)
            FAIL(ANSFM_ERR_INVALID, "map2xvec: no device-resident map2pro result of these dimensions");
        dA = ctx->map_out.as<double>();
    }
    HIPCHK(ctx->map_b.reserve(nxm * D));
    HIPCHK(hipMemcpyAsync(ctx->map_b.p, xmap, nxm * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx->tmp_out.reserve(nout * D));
    std::vector<GemmBatch> batch;
    for (int p = 0; p < P; ++p) batch.push_back(GemmBatch{(long long)p, 0, (long long)p * NX});
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.A = dA; g.B = ctx->map_b.as<double>(); g.C = ctx->tmp_out.as<double>();
    g.M = W; g.N = NX; g.K = NPAR * NPRO;
    g.a_sm = (long long)NPAR * NPRO * P; g.a_sk = P;
    g.b_sk = 1; g.b_sn = (long long)NPAR * NPRO;
    g.c_sm = (long long)P * NX; g.c_sn = 1;
    int rc = launch_gemm(ctx, g, batch);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dSPECOUT, ctx->tmp_out.p, nout * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}


/* ------------------------------------------------------------------------------------------ */
/* ILS convolution (Measurement_0.lblconv / lblconvg / lblconv_fil / lblconvg_fil, *_ngeom)    */
/* ------------------------------------------------------------------------------------------ */
static int ils_conv_impl(ansfm_ctx *ctx, int nwave, const double *vwave, int ny, const double *y, int nx, const double *dydx,
                         int nconv, const double *vconv, int ishape, double fwhm, int hamming_rule, int nfilmax,
                         const int32_t *nfil, const double *vfil, const double *afil, double *yout, double *gradout,
                         bool bracket = false, bool integrate = false)
{
    CHECK_CTX(ctx);
    const bool filter = nfil != nullptr;
    if (nwave <= 0 || nconv <= 0 || nx < 0 || ny <= 0 || !vwave || !y || !vconv || !yout || (nx > 0 && (!dydx || !gradout)) ||
        (filter && (!vfil || !afil || nfilmax < 2)))
        FAIL(ANSFM_ERR_INVALID, "lblconv: bad argument");
    for (int i = 1; i < nwave; ++i)
        if (!(vwave[i] >= vwave[i - 1])) FAIL(ANSFM_ERR_UNSORTED, "lblconv: the calculation wavenumbers must be ascending");
    if (filter)
        for (int j = 0; j < nconv; ++j) {
            if (nfil[j] < 2 || nfil[j] > nfilmax) FAIL(ANSFM_ERR_INVALID, "lblconv_fil: 2 <= nfil[j] <= rows of vfil");
            for (int k = 1; k < nfil[j]; ++k)
                if (!(vfil[(size_t)k * nconv + j] > vfil[(size_t)(k - 1) * nconv + j]))
                    FAIL(ANSFM_ERR_UNSORTED, "lblconv_fil: filter wavenumbers must be strictly ascending");
            if (bracket && (!(vwave[0] < vfil[j]) || !(vwave[nwave - 1] > vfil[(size_t)(nfil[j] - 1) * nconv + j])))
                FAIL(ANSFM_ERR_INVALID, "conv: every filter must lie strictly inside the calculation grid (the reference "
                                        "raises IndexError otherwise)");
        }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double);
    ConvParams p;
    memset(&p, 0, sizeof p);
    Stager st{ctx};
    p.vwave = st.up(vwave, nwave); p.y = st.up(y, (size_t)nwave * ny); p.dydx = st.up(dydx, (size_t)nwave * nx);
    p.vconv = st.up(vconv, nconv);
    if (filter) {
        p.nfil = st.up(nfil, nconv); p.vfil = st.up(vfil, (size_t)nfilmax * nconv); p.afil = st.up(afil, (size_t)nfilmax * nconv);
    }
    if (st.rc) return st.rc;
    HIPCHK(ctx->tmp_out.reserve(((size_t)nconv * (nx + ny)) * D));
    p.yout = ctx->tmp_out.as<double>(); p.gradout = p.yout + (size_t)nconv * ny;
    p.nwave = nwave; p.nx = nx; p.ny = ny; p.nconv = nconv; p.ishape = ishape; p.hamming_rule = hamming_rule;
    p.filter = filter ? (integrate ? 3 : bracket ? 2 : 1) : 0;
    p.fwhm = fwhm;
    hipLaunchKernelGGL(k_ils_conv, dim3((unsigned)nconv, (unsigned)((nx + ny + 127) / 128)), dim3(128), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(yout, p.yout, (size_t)nconv * ny * D, hipMemcpyDeviceToHost, ctx->stream));
    if (nx > 0) HIPCHK(hipMemcpyAsync(gradout, p.gradout, (size_t)nconv * nx * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_lblconv(ansfm_ctx *ctx, int nwave, const double *vwave, const double *y, int nx, const double *dydx, int nconv,
                  const double *vconv, int ishape, double fwhm, double *yout, double *gradout)
{
    if (ctx && !(fwhm > 0.0)) FAIL(ANSFM_ERR_INVALID, "lblconv: only valid if FWHM > 0");
    return ils_conv_impl(ctx, nwave, vwave, 1, y, nx, dydx, nconv, vconv, ishape, fwhm, nx > 0 ? 1 : 0, 0, nullptr, nullptr,
                         nullptr, yout, gradout);
}

int ansfm_lblconv_ngeom(ansfm_ctx *ctx, int nwave, const double *vwave, int ngeom, const double *y, int nx,
                        const double *dydx, int nconv, const double *vconv, int ishape, double fwhm, double *yout,
                        double *gradout)
{
    if (ctx && (!(fwhm > 0.0) || ngeom <= 0)) FAIL(ANSFM_ERR_INVALID, "lblconv_ngeom: only valid if FWHM > 0, NGEOM > 0");
    return ils_conv_impl(ctx, nwave, vwave, ngeom, y, ngeom * nx, dydx, nconv, vconv, ishape, fwhm, 2, 0, nullptr, nullptr,
                         nullptr, yout, gradout);
}

int ansfm_lblconv_fil(ansfm_ctx *ctx, int nwave, const double *vwave, const double *y, int nx, const double *dydx, int nconv,
                      const double *vconv, int nfilmax, const int32_t *nfil, const double *vfil, const double *afil,
                      double *yout, double *gradout)
{
    if (ctx && !nfil) FAIL(ANSFM_ERR_INVALID, "lblconv_fil: bad argument");
    return ils_conv_impl(ctx, nwave, vwave, 1, y, nx, dydx, nconv, vconv, 0, 0.0, 0, nfilmax, nfil, vfil, afil, yout, gradout);
}

int ansfm_conv_fil(ansfm_ctx *ctx, int nwave, const double *vwave, const double *y, int nx, const double *dydx, int nconv,
                   const double *vconv, int nfilmax, const int32_t *nfil, const double *vfil, const double *afil,
                   double *yout, double *gradout)
{
    if (ctx && !nfil) FAIL(ANSFM_ERR_INVALID, "conv_fil: bad argument");
    return ils_conv_impl(ctx, nwave, vwave, 1, y, nx, dydx, nconv, vconv, 0, 0.0, 0, nfilmax, nfil, vfil, afil, yout, gradout,
                         true);
}

int ansfm_integrate_filter(ansfm_ctx *ctx, int nwave, const double *vwave, int ngeom, const double *y, int nx,
                           const double *dydx, int nconv, const double *vconv, int nfilmax, const int32_t *nfil,
                           const double *vfil, const double *afil, double *yout, double *gradout)
{
    if (ctx && (!nfil || ngeom <= 0)) FAIL(ANSFM_ERR_INVALID, "integrate_filter: bad argument");
    return ils_conv_impl(ctx, nwave, vwave, ngeom, y, ngeom * nx, dydx, nconv, vconv, 0, 0.0, 0, nfilmax, nfil, vfil, afil,
                         yout, gradout, false, true);
}

int ansfm_lblconv_fil_ngeom(ansfm_ctx *ctx, int nwave, const double *vwave, int ngeom, const double *y, int nx,
                            const double *dydx, int nconv, const double *vconv, int nfilmax, const int32_t *nfil,
                            const double *vfil, const double *afil, double *yout, double *gradout)
{
    if (ctx && (!nfil || ngeom <= 0)) FAIL(ANSFM_ERR_INVALID, "lblconv_fil_ngeom: bad argument");
    return ils_conv_impl(ctx, nwave, vwave, ngeom, y, ngeom * nx, dydx, nconv, vconv, 0, 0.0, 0, nfilmax, nfil, vfil, afil,
                         yout, gradout);
}


/* ------------------------------------------------------------------------------------------ */
/* continuum: collision-induced absorption (ForwardModel_0.calc_tau_cia)                       */
/* ------------------------------------------------------------------------------------------ */
int ansfm_calc_tau_cia(ansfm_ctx *ctx, int W, const double *WAVEN, int NWC, const double *cia_waven, int NPAIR, int NPE,
                       int NT, const double *K_CIA, const double *cia_temp, int nfrac, const double *cia_frac, int NPARA,
                       const int32_t *igas1, const int32_t *igas2, int L, int NVMR, const double *lay_temp,
                       const double *lay_frac, const double *q, const double *xfac, int ico2, const double *k_co2, int in2,
                       const double *k_n2n2, int ih2, const double *k_n2h2, double *TAUCIA, double *dTAUCIA)
{
    CHECK_CTX(ctx);
    if (W <= 0 || NWC < 2 || NPAIR < 0 || NPE < 1 || NT < 2 || nfrac < 1 || L <= 0 || NVMR < 2 || !WAVEN || !cia_waven ||
        !K_CIA || !cia_temp || !cia_frac || (NPAIR > 0 && (!igas1 || !igas2)) || !lay_temp || !lay_frac || !q || !xfac ||
        !TAUCIA || (ico2 >= 0 && !k_co2) || (in2 >= 0 && !k_n2n2) || (in2 >= 0 && ih2 >= 0 && !k_n2h2) ||
        ico2 >= NVMR || in2 >= NVMR || ih2 >= NVMR)
        FAIL(ANSFM_ERR_INVALID, "calc_tau_cia: bad argument");
    for (int i = 0; i < NPAIR; ++i)
        if (igas1[i] >= NVMR || igas2[i] >= NVMR) FAIL(ANSFM_ERR_INVALID, "calc_tau_cia: pair gas index outside the atmosphere");
    for (int i = 1; i < W; ++i)
        if (!(WAVEN[i] >= WAVEN[i - 1])) FAIL(ANSFM_ERR_UNSORTED, "calc_tau_cia: wavenumbers must be ascending");
    // per-layer brackets and weights (:4588-4666), including the reference's overwrite of temp1 in the upper
    // para-fraction clamp (:4623)
    std::vector<CiaLayer> lay(L);
    for (int l = 0; l < L; ++l) {
        const CiaLayer c = cia_layer(lay_temp[l], lay_frac[l], xfac[l], NT, cia_temp, nfrac, cia_frac, NPARA);
        if (c.ipl < 0 || c.iphi < 0 || c.ipl >= NPE || c.iphi >= NPE || (nfrac > 1 && c.iphi >= nfrac))
            FAIL(ANSFM_ERR_INVALID, "calc_tau_cia: para-H2 bracket outside K_CIA (the reference raises IndexError here)");
        lay[l] = c;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double);
    double cmin = cia_waven[0], cmax = cia_waven[0];
    for (int i = 1; i < NWC; ++i) { cmin = std::min(cmin, cia_waven[i]); cmax = std::max(cmax, cia_waven[i]); }
    const int covers = (cmin <= WAVEN[0] && cmax >= WAVEN[W - 1]) ? 1 : 0;      // :4671
    CiaParams p;
    memset(&p, 0, sizeof p);
    Stager st{ctx};
    p.waven = st.up(WAVEN, W); p.cia_waven = st.up(cia_waven, NWC); p.K = st.up(K_CIA, (size_t)NPAIR * NPE * NT * NWC);
    p.lay = st.up(lay.data(), L); p.g1 = st.up(igas1, NPAIR); p.g2 = st.up(igas2, NPAIR); p.q = st.up(q, (size_t)L * NVMR);
    p.k_co2 = st.up(ico2 >= 0 ? k_co2 : nullptr, W); p.k_n2n2 = st.up(in2 >= 0 ? k_n2n2 : nullptr, W);
    p.k_n2h2 = st.up((in2 >= 0 && ih2 >= 0) ? k_n2h2 : nullptr, W);
    if (st.rc) return st.rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));                     // `lay` is a host temporary
    const size_t nt = (size_t)W * L, nd = dTAUCIA ? nt * (NVMR + 2) : 0;
    HIPCHK(ctx->tmp_out.reserve((nt + nd) * D));
    p.tau = ctx->tmp_out.as<double>(); p.dtau = dTAUCIA ? p.tau + nt : nullptr;
    p.W = W; p.NWC = NWC; p.NPAIR = NPAIR; p.NPE = NPE; p.NT = NT; p.L = L; p.NVMR = NVMR; p.covers = covers;
    p.ico2 = ico2; p.in2 = in2; p.ih2 = ih2;
    if (p.dtau) HIPCHK(hipMemsetAsync(p.dtau, 0, nd * D, ctx->stream));
    hipLaunchKernelGGL(k_tau_cia, dim3(nblk((size_t)W, 128), (unsigned)L), dim3(128), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(TAUCIA, p.tau, nt * D, hipMemcpyDeviceToHost, ctx->stream));
    if (dTAUCIA) HIPCHK(hipMemcpyAsync(dTAUCIA, p.dtau, nd * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* continuum: Rayleigh scattering (ForwardModel_0.calc_tau_rayleigh) and aerosols (calc_tau_dust) */
/* ------------------------------------------------------------------------------------------ */
int ansfm_calc_tau_rayleigh(ansfm_ctx *ctx, int mode, int ISPACE, int W, const double *WAVEC, int L, const double *TOTAM,
                            const double *f4, double *TAURAY, double *dTAURAY)
{
    CHECK_CTX(ctx);
    if (W <= 0 || L <= 0 || !WAVEC || !TOTAM || !TAURAY || !dTAURAY || (ISPACE != 0 && ISPACE != 1) ||
        (mode != 1 && mode != 2 && mode != 4 && mode != 12) || (mode == 4 && !f4))
        FAIL(ANSFM_ERR_INVALID, "calc_tau_rayleigh: bad argument (mode = IRAY 1, 2, 4 or 12 for calc_tau_rayleighv)");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double), nt = (size_t)W * L;
    RayParams p;
    memset(&p, 0, sizeof p);
    Stager st{ctx};
    p.wavec = st.up(WAVEC, W); p.totam = st.up(TOTAM, L); p.f4 = st.up(f4, mode == 4 ? (size_t)L * 4 : 0);
    if (st.rc) return st.rc;
    HIPCHK(ctx->tmp_out.reserve(2 * nt * D));
    p.tau = ctx->tmp_out.as<double>(); p.dtau = p.tau + nt;
    p.W = W; p.L = L; p.mode = mode; p.ispace = ISPACE;
    hipLaunchKernelGGL(k_tau_rayleigh, dim3(nblk((size_t)W * L, 128)), dim3(128), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(TAURAY, p.tau, nt * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(dTAURAY, p.dtau, nt * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

static int rayleigh_batch_impl(ansfm_ctx *ctx, int mode, int ISPACE, int n_models, int L, const double *TOTAM,
                               const double *f4, double *TAURAY_dev, bool dev_in);

int ansfm_calc_tau_rayleigh_batch_dev(ansfm_ctx *ctx, int mode, int ISPACE, int n_models, int L, const double *TOTAM,
                                      const double *f4, double *TAURAY_dev)
{
    return rayleigh_batch_impl(ctx, mode, ISPACE, n_models, L, TOTAM, f4, TAURAY_dev, false);
}

int ansfm_calc_tau_rayleigh_batch_dev_in(ansfm_ctx *ctx, int mode, int ISPACE, int n_models, int L, const double *TOTAM_dev,
                                         const double *f4_dev, double *TAURAY_dev)
{
    return rayleigh_batch_impl(ctx, mode, ISPACE, n_models, L, TOTAM_dev, f4_dev, TAURAY_dev, true);
}

static int rayleigh_batch_impl(ansfm_ctx *ctx, int mode, int ISPACE, int n_models, int L, const double *TOTAM,
                               const double *f4, double *TAURAY_dev, bool dev_in)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "calc_tau_rayleigh_batch_dev: upload a table first (its wavenumber grid is used)");
    if (n_models <= 0 || L <= 0 || !TOTAM || !TAURAY_dev || (ISPACE != 0 && ISPACE != 1) ||
        (mode != 1 && mode != 2 && mode != 4 && mode != 12) || (mode == 4 && !f4))
        FAIL(ANSFM_ERR_INVALID, "calc_tau_rayleigh_batch_dev: bad argument (mode = IRAY 1, 2, 4 or 12 for calc_tau_rayleighv)");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double), nl = (size_t)n_models * L;
    RayParams p;
    memset(&p, 0, sizeof p);
    if (dev_in) { p.totam = TOTAM; p.f4 = (mode == 4) ? f4 : nullptr; }
    else {
        Stager st{ctx, 1};
        p.totam = st.up(TOTAM, nl); p.f4 = st.up(f4, mode == 4 ? nl * 4 : 0);
        if (st.rc) return st.rc;
    }
    p.wavec = ctx->d_wave.as<double>();
    p.tau = TAURAY_dev; p.dtau = nullptr;
    p.W = ctx->W; p.L = (int)nl; p.mode = mode; p.ispace = ISPACE; p.Lm = L;
    hipLaunchKernelGGL(k_tau_rayleigh, dim3(nblk((size_t)ctx->W * nl, 128)), dim3(128), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    if (!dev_in) HIPCHK(hipStreamSynchronize(ctx->stream));       // the host staging buffers are reused by the next call
    return ANSFM_OK;
}

// not-a-knot cubic spline through (x, y[stride]) : per interval b, c, d of  y_a + t (b + t (c + t d)),  t = x - x_a
static void notaknot_coeffs(int n, const double *x, const double *y, size_t stride, double *coef)
{
    std::vector<double> h(n - 1), s(n - 1), M(n, 0.0);
    for (int i = 0; i < n - 1; ++i) { h[i] = x[i + 1] - x[i]; s[i] = (y[(size_t)(i + 1) * stride] - y[(size_t)i * stride]) / h[i]; }
    // unknowns M_1..M_{n-2} (second derivatives); M_0 and M_{n-1} eliminated with the not-a-knot conditions
    const int m = n - 2;
    std::vector<double> lo(m, 0.0), di(m, 0.0), up(m, 0.0), r(m, 0.0);
    for (int k = 0; k < m; ++k) {
        const int i = k + 1;
        lo[k] = h[i - 1]; di[k] = 2.0 * (h[i - 1] + h[i]); up[k] = h[i];
        r[k] = 6.0 * (s[i] - s[i - 1]);
    }
    if (m == 1) {   // n == 3 is refused by the caller; kept total
        M[1] = r[0] / di[0];
    } else {
        // M_0 = ((h0+h1) M_1 - h0 M_2) / h1 ;  M_{n-1} = ((h_{n-2}+h_{n-3}) M_{n-2} - h_{n-2} M_{n-3}) / h_{n-3}
        const double h0 = h[0], h1 = h[1], hn = h[n - 2], hm = h[n - 3];
        di[0] += lo[0] * (h0 + h1) / h1; up[0] -= lo[0] * h0 / h1; lo[0] = 0.0;
        di[m - 1] += up[m - 1] * (hn + hm) / hm; lo[m - 1] -= up[m - 1] * hn / hm; up[m - 1] = 0.0;
        for (int k = 1; k < m; ++k) {   // Thomas
            const double f = lo[k] / di[k - 1];
            di[k] -= f * up[k - 1];
            r[k] -= f * r[k - 1];
        }
        M[m] = r[m - 1] / di[m - 1];
        for (int k = m - 2; k >= 0; --k) M[k + 1] = (r[k] - up[k] * M[k + 2]) / di[k];
        M[0] = ((h0 + h1) * M[1] - h0 * M[2]) / h1;
        M[n - 1] = ((hn + hm) * M[n - 2] - hn * M[n - 3]) / hm;
    }
    for (int i = 0; i < n - 1; ++i) {
        coef[(size_t)i * 3 + 0] = s[i] - h[i] * (2.0 * M[i] + M[i + 1]) / 6.0;
        coef[(size_t)i * 3 + 1] = M[i] / 2.0;
        coef[(size_t)i * 3 + 2] = (M[i + 1] - M[i]) / (6.0 * h[i]);
    }
}

int ansfm_calc_tau_dust(ansfm_ctx *ctx, int W, const double *WAVEC, int NWS, const double *SWAVE, int NDUST,
                        const double *KEXT, const double *KSCA, int L, const double *CONT, double *TAUDUST,
                        double *TAUCLSCAT, double *dTAUDUSTdq, double *dTAUCLSCATdq)
{
    CHECK_CTX(ctx);
    if (W <= 0 || NWS < 2 || NDUST <= 0 || L <= 0 || !WAVEC || !SWAVE || !KEXT || !KSCA || !CONT || !TAUDUST || !TAUCLSCAT ||
        !dTAUDUSTdq || !dTAUCLSCATdq)
        FAIL(ANSFM_ERR_INVALID, "calc_tau_dust: bad argument");
    if (NWS == 3) FAIL(ANSFM_ERR_UNSUPPORTED, "calc_tau_dust: three tabulated wavelengths (scipy's cubic interp1d refuses them too)");
    for (int i = 1; i < NWS; ++i)
        if (!(SWAVE[i] > SWAVE[i - 1])) FAIL(ANSFM_ERR_UNSORTED, "calc_tau_dust: Scatter.WAVE must be strictly ascending");
    for (int w = 0; w < W; ++w)      // interp1d(bounds_error=True)
        if (!(WAVEC[w] >= SWAVE[0] && WAVEC[w] <= SWAVE[NWS - 1]))
            FAIL(ANSFM_ERR_INVALID, "calc_tau_dust: a calculation wavenumber is outside the range of the aerosol properties");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double), nt = (size_t)W * L * NDUST;
    const int cubic = NWS > 2;
    std::vector<double> coef;
    if (cubic) {
        coef.resize((size_t)2 * NDUST * (NWS - 1) * 3);
        for (int i = 0; i < NDUST; ++i) {
            notaknot_coeffs(NWS, SWAVE, KEXT + i, NDUST, coef.data() + (size_t)i * (NWS - 1) * 3);
            notaknot_coeffs(NWS, SWAVE, KSCA + i, NDUST, coef.data() + ((size_t)NDUST + i) * (NWS - 1) * 3);
        }
    }
    DustParams p;
    memset(&p, 0, sizeof p);
    Stager st{ctx};
    p.wavec = st.up(WAVEC, W); p.swave = st.up(SWAVE, NWS); p.kext = st.up(KEXT, (size_t)NWS * NDUST);
    p.ksca = st.up(KSCA, (size_t)NWS * NDUST); p.cont = st.up(CONT, (size_t)L * NDUST);
    p.cext = st.up(cubic ? coef.data() : nullptr, coef.size());
    if (st.rc) return st.rc;
    HIPCHK(ctx->tmp_out.reserve(4 * nt * D));
    p.csca = p.cext ? p.cext + (size_t)NDUST * (NWS - 1) * 3 : nullptr;
    p.taudust = ctx->tmp_out.as<double>(); p.tauclscat = p.taudust + nt; p.dtaudust = p.tauclscat + nt; p.dtauclscat = p.dtaudust + nt;
    p.W = W; p.NWS = NWS; p.NDUST = NDUST; p.L = L; p.cubic = cubic;
    hipLaunchKernelGGL(k_tau_dust, dim3(nblk((size_t)W, 128), (unsigned)NDUST), dim3(128), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(TAUDUST, p.taudust, nt * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(TAUCLSCAT, p.tauclscat, nt * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(dTAUDUSTdq, p.dtaudust, nt * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(dTAUCLSCATdq, p.dtauclscat, nt * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* continuum sources resident in the context, on the uploaded table's grid                     */
/* ------------------------------------------------------------------------------------------ */
int ansfm_upload_cia(ansfm_ctx *ctx, int ISPACE, int NWC, const double *cia_waven, int NPAIR, int NPE, int NT, const double *K_CIA,
                     const double *cia_temp, int nfrac, const double *cia_frac, int NPARA, const int32_t *igas1,
                     const int32_t *igas2, int NVMR, int ico2, const double *k_co2, int in2, const double *k_n2n2, int ih2,
                     const double *k_n2h2)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "upload_cia: upload a table first (the source lives on its wavenumber grid)");
    if ((ISPACE != 0 && ISPACE != 1) || NWC < 2 || NPAIR < 0 || NPE < 1 || NT < 2 || nfrac < 1 || NPARA < 0 || NVMR < 2 ||
        !cia_waven || !K_CIA || !cia_temp || !cia_frac || (NPAIR > 0 && (!igas1 || !igas2)) || (ico2 >= 0 && !k_co2) ||
        (in2 >= 0 && !k_n2n2) || (in2 >= 0 && ih2 >= 0 && !k_n2h2) || ico2 >= NVMR || in2 >= NVMR || ih2 >= NVMR)
        FAIL(ANSFM_ERR_INVALID, "upload_cia: bad argument");
    for (int i = 0; i < NPAIR; ++i)
        if (igas1[i] >= NVMR || igas2[i] >= NVMR) FAIL(ANSFM_ERR_INVALID, "upload_cia: pair gas index outside the atmosphere");
    // a layer's para-H2 bracket must stay inside K_CIA whatever its fraction is: the per-layer IndexError of ansfm_calc_tau_cia
    // then cannot arise on the device
    if (NPARA > 0 && !(NPARA == nfrac && nfrac == NPE && NPE >= 2))
        FAIL(ANSFM_ERR_UNSUPPORTED, "upload_cia: a para-H2 table needs NPARA == len(FRAC) == K_CIA.shape[1] >= 2 (use ansfm_calc_tau_cia)");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W;
    // the table is evaluated at x = WAVE (ISPACE 0) or 1e4 / WAVE (ISPACE 1, :4565); covers (:4671) on the range of that x
    double xmin = ctx->h_wave[0], xmax = ctx->h_wave[0];
    for (int w = 0; w < W; ++w) {
        const double x = ISPACE == 0 ? ctx->h_wave[w] : 1.e4 / ctx->h_wave[w];
        if (w == 0) { xmin = xmax = x; } else { xmin = std::min(xmin, x); xmax = std::max(xmax, x); }
    }
    double cmin = cia_waven[0], cmax = cia_waven[0];
    for (int i = 1; i < NWC; ++i) { cmin = std::min(cmin, cia_waven[i]); cmax = std::max(cmax, cia_waven[i]); }
    const size_t nK = (size_t)NPAIR * NPE * NT * NWC, D = sizeof(double);
    const size_t total = (size_t)NWC + nK + NT + nfrac + 3 * (size_t)W;
    ctx->cia_on = 0;
    HIPCHK(ctx->cia_tab.reserve(total * D));
    HIPCHK(ctx->cia_idx.reserve(std::max<size_t>(1, 2 * (size_t)NPAIR) * sizeof(int32_t)));
    double *d = ctx->cia_tab.as<double>();
    auto put = [&](const double *src, size_t count, bool have) -> hipError_t {
        hipError_t e = have ? hipMemcpyAsync(d, src, count * D, hipMemcpyHostToDevice, ctx->stream)
                            : hipMemsetAsync(d, 0, count * D, ctx->stream);
        d += count;
        return e;
    };
    HIPCHK(put(cia_waven, NWC, true)); HIPCHK(put(K_CIA, nK, nK > 0)); HIPCHK(put(cia_temp, NT, true));
    HIPCHK(put(cia_frac, nfrac, true));
    HIPCHK(put(k_co2, W, ico2 >= 0)); HIPCHK(put(k_n2n2, W, in2 >= 0)); HIPCHK(put(k_n2h2, W, in2 >= 0 && ih2 >= 0));
    if (NPAIR > 0) {
        HIPCHK(hipMemcpyAsync(ctx->cia_idx.p, igas1, NPAIR * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->cia_idx.as<int32_t>() + NPAIR, igas2, NPAIR * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));                     // the caller's arrays are free again
    ctx->cia_ispace = ISPACE; ctx->cia_NWC = NWC; ctx->cia_NPAIR = NPAIR; ctx->cia_NPE = NPE; ctx->cia_NT = NT;
    ctx->cia_nfrac = nfrac; ctx->cia_NPARA = NPARA; ctx->cia_NVMR = NVMR; ctx->cia_ico2 = ico2; ctx->cia_in2 = in2; ctx->cia_ih2 = ih2;
    ctx->cia_covers = (cmin <= xmin && cmax >= xmax) ? 1 : 0;
    ctx->cia_on = 1;
    return ANSFM_OK;
}

int ansfm_upload_dust(ansfm_ctx *ctx, int NWS, const double *SWAVE, int NDUST, const double *KEXT, const double *KSCA)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "upload_dust: upload a table first (the source lives on its wavenumber grid)");
    if (NWS < 2 || NDUST <= 0 || !SWAVE || !KEXT) FAIL(ANSFM_ERR_INVALID, "upload_dust: bad argument");
    if (NDUST > 7)
        FAIL(ANSFM_ERR_UNSUPPORTED, "upload_dust: more than 7 aerosol populations (NumPy sums 8 and more pairwise; use ansfm_calc_tau_dust)");
    if (NWS == 3) FAIL(ANSFM_ERR_UNSUPPORTED, "upload_dust: three tabulated wavelengths (scipy's cubic interp1d refuses them too)");
    for (int i = 1; i < NWS; ++i)
        if (!(SWAVE[i] > SWAVE[i - 1])) FAIL(ANSFM_ERR_UNSORTED, "upload_dust: Scatter.WAVE must be strictly ascending");
    const int W = ctx->W, Wpad = ctx->Wpad;
    for (int w = 0; w < W; ++w)      // interp1d(bounds_error=True)
        if (!(ctx->h_wave[w] >= SWAVE[0] && ctx->h_wave[w] <= SWAVE[NWS - 1]))
            FAIL(ANSFM_ERR_INVALID, "upload_dust: a wavenumber of the table is outside the range of the aerosol properties");
    HIPCHK(hipSetDevice(ctx->device));
    // the scattering cross sections decide where the linear interpolant replaces the spline (:4849-4851); without them: zeros
    const size_t nk = (size_t)NWS * NDUST;
    std::vector<double> zeros;
    if (!KSCA) { zeros.assign(nk, 0.0); KSCA = zeros.data(); }
    const int cubic = NWS > 2;
    std::vector<double> coef;
    if (cubic) {
        coef.resize((size_t)2 * NDUST * (NWS - 1) * 3);
        for (int i = 0; i < NDUST; ++i) {
            notaknot_coeffs(NWS, SWAVE, KEXT + i, NDUST, coef.data() + (size_t)i * (NWS - 1) * 3);
            notaknot_coeffs(NWS, SWAVE, KSCA + i, NDUST, coef.data() + ((size_t)NDUST + i) * (NWS - 1) * 3);
        }
    }
    ctx->dust_n = 0;
    DustParams p;
    memset(&p, 0, sizeof p);
    Stager st{ctx};
    p.swave = st.up(SWAVE, NWS); p.kext = st.up(KEXT, nk); p.ksca = st.up(KSCA, nk);
    p.cext = st.up(cubic ? coef.data() : nullptr, coef.size());
    if (st.rc) return st.rc;
    p.csca = p.cext ? p.cext + (size_t)NDUST * (NWS - 1) * 3 : nullptr;
    p.wavec = ctx->d_wave.as<double>();
    p.W = W; p.NWS = NWS; p.NDUST = NDUST; p.cubic = cubic;
    HIPCHK(ctx->dust_kext.reserve((size_t)NDUST * Wpad * sizeof(double)));
    HIPCHK(ctx->dust_ksca.reserve((size_t)NDUST * Wpad * sizeof(double)));
    hipLaunchKernelGGL(k_dust_kext_grid, dim3(nblk((size_t)Wpad, 128), (unsigned)NDUST), dim3(128), 0, ctx->stream, p, Wpad,
                       ctx->dust_kext.as<double>(), ctx->dust_ksca.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));                     // the coefficients are host temporaries
    ctx->dust_n = NDUST;
    return ANSFM_OK;
}

int ansfm_clear_continuum_sources(ansfm_ctx *ctx)
{
    CHECK_CTX(ctx);
    clear_continuum_sources(ctx);
    return ANSFM_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* k-table generator: k-distribution of an LBL spectrum in bins (Spectroscopy_0.calc_ktable_chunk) */
/* ------------------------------------------------------------------------------------------ */
int ansfm_kdist_bins(ansfm_ctx *ctx, int ncalc, const double *wavecalc, const double *kabs, int nbin, const double *vbinmin,
                     const double *vbinmax, const double *wcen, int nfilmax, const int32_t *nfil, const double *dfil,
                     const double *afil, int NG, const double *g_ord, double *kout)
{
    CHECK_CTX(ctx);
    if (ncalc < 2 || nbin <= 0 || NG <= 0 || !wavecalc || !kabs || !vbinmin || !vbinmax || !g_ord || !kout ||
        (nfil && (!dfil || !afil || !wcen || nfilmax < 1)))
        FAIL(ANSFM_ERR_INVALID, "kdist_bins: bad argument");
    for (int i = 1; i < ncalc; ++i)
        if (!(wavecalc[i] > wavecalc[i - 1])) FAIL(ANSFM_ERR_UNSORTED, "kdist_bins: the line-by-line grid must be ascending");
    // mask = (wavecalc >= vbinmin) & (wavecalc <= vbinmax)   (:3633)
    std::vector<int32_t> i0(nbin);
    std::vector<int64_t> off(nbin + 1, 0);
    for (int b = 0; b < nbin; ++b) {
        const long a = (long)(std::lower_bound(wavecalc, wavecalc + ncalc, vbinmin[b]) - wavecalc);
        const long e = (long)(std::upper_bound(wavecalc, wavecalc + ncalc, vbinmax[b]) - wavecalc);
        if (e <= a) FAIL(ANSFM_ERR_INVALID, "kdist_bins: a bin holds no line-by-line point (np.interp would raise on the empty sample)");
        if (nfil && (nfil[b] < 1 || nfil[b] > nfilmax)) FAIL(ANSFM_ERR_INVALID, "kdist_bins: 1 <= nfil[bin] <= rows of the filter arrays");
        i0[b] = (int32_t)a;
        off[b + 1] = off[b] + (e - a);
    }
    const int64_t total = off[nbin];
    if (total > 0x7fffffffLL) FAIL(ANSFM_ERR_UNSUPPORTED, "kdist_bins: more than 2^31 points in one call; split the bins");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double);
    KdistParams p;
    memset(&p, 0, sizeof p);
    Stager st{ctx};
    p.wavecalc = st.up(wavecalc, ncalc); p.kabs = st.up(kabs, ncalc); p.i0 = st.up(i0.data(), nbin);
    p.off = st.up(off.data(), nbin + 1); p.g_ord = st.up(g_ord, NG);
    if (nfil) {
        p.wcen = st.up(wcen, nbin); p.nfil = st.up(nfil, nbin); p.dfil = st.up(dfil, (size_t)nfilmax * nbin);
        p.afil = st.up(afil, (size_t)nfilmax * nbin);
    }
    if (st.rc) return st.rc;
    HIPCHK(ctx->tmp_in.reserve((size_t)total * D));
    HIPCHK(ctx->tmp_in2.reserve((size_t)total * D));
    HIPCHK(ctx->tmp_out.reserve((size_t)nbin * NG * D));
    p.keys = ctx->tmp_in.as<double>(); p.vals = ctx->tmp_in2.as<double>(); p.kout = ctx->tmp_out.as<double>();
    p.dv = wavecalc[1] - wavecalc[0];                                     // delvarray (:3647)
    p.nbin = nbin; p.NG = NG;
    const int herr = ansfm_kdist_run((void *)ctx->stream, p, total);
    if (herr != 0) FAIL(ANSFM_ERR_HIP, std::string("kdist_bins: ") + hipGetErrorString((hipError_t)herr));
    HIPCHK(hipMemcpyAsync(kout, p.kout, (size_t)nbin * NG * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* layering                                                                                    */
/* ------------------------------------------------------------------------------------------ */
static int layer_average_impl(ansfm_ctx *ctx, int n_models, double RADIUS, int NPRO, const double *H, const double *P,
                              const double *T, int NVMR, const double *VMR, int NDUST, const double *DUST,
                              const double *PARAH2, int NLAY, const double *BASEH, double LAYANG, int LAYINT, double LAYHT,
                              int NINT, const int32_t *DUST_UNITS, const double *XMOLWT, double *HEIGHT, double *PRESS,
                              double *TEMP, double *TOTAM, double *AMOUNT, double *PP, double *CONT, double *FRAC,
                              double *DELH, double *BASET, double *LAYSF, bool with_grad, double *DTE, double *DAM,
                              double *DCO, double *DPH, double *dev_out = nullptr)
{
    // dev_out != nullptr: H .. XMOLWT and BASEH are DEVICE arrays and the results stay in dev_out (layout of
    // ansfm_layer_average_dev); the host result pointers are not used
    CHECK_CTX(ctx);
    const bool dev = dev_out != nullptr;
    if (dev) HEIGHT = PRESS = TEMP = TOTAM = AMOUNT = PP = FRAC = DELH = BASET = LAYSF = CONT = dev_out;
    int any_units = 0;
    if (DUST_UNITS) for (int j = 0; j < NDUST; ++j) if (DUST_UNITS[j] == -1) any_units = 1;
    if (with_grad) {
        if (!DTE || !DAM || !DCO || !DPH) FAIL(ANSFM_ERR_INVALID, "layer_averageg: bad argument");
        if ((NINT % 2) == 0) FAIL(ANSFM_ERR_INVALID, "NINT must be odd for Simpson's rule.");            // Layer_0.py:1188
        if (LAYINT == 0 && any_units && NDUST > 0)
            FAIL(ANSFM_ERR_INVALID, "setting an array element with a sequence.");   // the reference's failure at :1255-1257
    }
    if (n_models <= 0 || NPRO < 2 || NVMR <= 0 || NDUST < 0 || NLAY <= 0 || !H || !P || !T || !VMR || !BASEH || !HEIGHT ||
        !PRESS || !TEMP || !TOTAM || !AMOUNT || !PP || !FRAC || !DELH || !BASET || !LAYSF || (NDUST > 0 && (!DUST || !CONT)) ||
        (LAYINT != 0 && LAYINT != 1))
        FAIL(ANSFM_ERR_INVALID, "layer_average: bad argument");
    if (LAYINT == 1 && (NINT < 2 || NINT > kLayMaxNint))
        FAIL(ANSFM_ERR_UNSUPPORTED, "layer_average: NINT must be in [2,256]");
    if (5 + 2 * NVMR + NDUST > 160) FAIL(ANSFM_ERR_UNSUPPORTED, "layer_average: 5 + 2*NVMR + NDUST <= 160");
    if (n_models > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "layer_average: at most 65535 states per call");
    if (DUST_UNITS && !XMOLWT)
        for (int j = 0; j < NDUST; ++j)
            if (DUST_UNITS[j] == -1) FAIL(ANSFM_ERR_INVALID, "if DUST_UNITS=-1 (particles per gram of atm), the XMOLWT must be defined");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double), n = n_models;
    LayerAvgParams p;
    memset(&p, 0, sizeof p);
    Stager st{ctx};
    auto in = [&](const double *a, size_t count) { return dev ? a : st.up(a, count); };   // device arrays stay where they are
    p.H = in(H, n * NPRO); p.P = in(P, n * NPRO); p.T = in(T, n * NPRO); p.VMR = in(VMR, n * NPRO * NVMR);
    p.DUST = in(DUST, n * NPRO * NDUST); p.PARAH2 = in(PARAH2, n * NPRO); p.XMOLWT = in(XMOLWT, n * NPRO);
    p.BASEH = in(BASEH, n * NLAY);
    st.slot = 8;                                                                    // the device route stages from here only
    p.dust_units = st.up(DUST_UNITS, NDUST);                                        // always a host array
    if (st.rc) return st.rc;
    const size_t nl = n * NLAY;
    const size_t tot = nl * (8 + 2 * (size_t)NVMR + NDUST) + (with_grad ? 4 * nl * NPRO : 0);
    if (!dev) HIPCHK(ctx->tmp_out.reserve(tot * D));
    double *o = dev ? dev_out : ctx->tmp_out.as<double>();
    p.HEIGHT = o; p.PRESS = o + nl; p.TEMP = o + 2 * nl; p.TOTAM = o + 3 * nl; p.FRAC = o + 4 * nl; p.DELH = o + 5 * nl;
    p.BASET = o + 6 * nl; p.LAYSF = o + 7 * nl; p.AMOUNT = o + 8 * nl; p.PP = p.AMOUNT + nl * NVMR; p.CONT = p.PP + nl * NVMR;
    p.RADIUS = RADIUS; p.LAYANG = LAYANG; p.LAYHT = LAYHT;
    p.n_models = n_models; p.NPRO = NPRO; p.NVMR = NVMR; p.NDUST = NDUST; p.NLAY = NLAY; p.LAYINT = LAYINT; p.NINT = NINT;
    if (with_grad) {
        p.with_grad = 1; p.any_dust_units = any_units;
        p.DTE = p.CONT + nl * NDUST; p.DAM = p.DTE + nl * NPRO; p.DCO = p.DAM + nl * NPRO; p.DPH = p.DCO + nl * NPRO;
        HIPCHK(hipMemsetAsync(p.DTE, 0, 4 * nl * NPRO * D, ctx->stream));
    }
    // several states without gradients: state 0 first, then the others, which take state 0's layers where their levels agree
    static const bool share_off = [] { const char *e = getenv("ANSFM_LAYER_SHARE"); return e && e[0] == '0'; }();
    if (n_models > 1 && !with_grad && !share_off) {
        hipLaunchKernelGGL(k_layer_average, dim3((unsigned)NLAY, 1u), dim3(128), 0, ctx->stream, p);
        HIPCHK(ctx->rt_same.reserve(nl));                 // (not in use at this point of a call sequence)
        unsigned char *flag = ctx->rt_same.as<unsigned char>();
        hipLaunchKernelGGL(k_layer_share, dim3(nblk(nl - NLAY, 128)), dim3(128), 0, ctx->stream, p, flag);
        p.m0 = 1; p.share = flag;
        hipLaunchKernelGGL(k_layer_average, dim3((unsigned)NLAY, (unsigned)(n_models - 1)), dim3(128), 0, ctx->stream, p);
    } else
        hipLaunchKernelGGL(k_layer_average, dim3((unsigned)NLAY, (unsigned)n_models), dim3(128), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    if (dev) {
        if (DUST_UNITS && NDUST > 0) HIPCHK(hipStreamSynchronize(ctx->stream));   // its staging buffer is reused by the next call
        return ANSFM_OK;
    }
    double *outs[8] = {HEIGHT, PRESS, TEMP, TOTAM, FRAC, DELH, BASET, LAYSF};
    for (int k = 0; k < 8; ++k) HIPCHK(hipMemcpyAsync(outs[k], o + k * nl, nl * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(AMOUNT, p.AMOUNT, nl * NVMR * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(PP, p.PP, nl * NVMR * D, hipMemcpyDeviceToHost, ctx->stream));
    if (NDUST > 0) HIPCHK(hipMemcpyAsync(CONT, p.CONT, nl * NDUST * D, hipMemcpyDeviceToHost, ctx->stream));
    if (with_grad) {
        double *mo[4] = {DTE, DAM, DCO, DPH};
        const double *ms[4] = {p.DTE, p.DAM, p.DCO, p.DPH};
        for (int k = 0; k < 4; ++k) HIPCHK(hipMemcpyAsync(mo[k], ms[k], nl * NPRO * D, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}


int ansfm_layer_average(ansfm_ctx *ctx, int n_models, double RADIUS, int NPRO, const double *H, const double *P,
                        const double *T, int NVMR, const double *VMR, int NDUST, const double *DUST, const double *PARAH2,
                        int NLAY, const double *BASEH, double LAYANG, int LAYINT, double LAYHT, int NINT,
                        const int32_t *DUST_UNITS, const double *XMOLWT, double *HEIGHT, double *PRESS, double *TEMP,
                        double *TOTAM, double *AMOUNT, double *PP, double *CONT, double *FRAC, double *DELH, double *BASET,
                        double *LAYSF)
{
    return layer_average_impl(ctx, n_models, RADIUS, NPRO, H, P, T, NVMR, VMR, NDUST, DUST, PARAH2, NLAY, BASEH, LAYANG, LAYINT,
                              LAYHT, NINT, DUST_UNITS, XMOLWT, HEIGHT, PRESS, TEMP, TOTAM, AMOUNT, PP, CONT, FRAC, DELH, BASET,
                              LAYSF, false, nullptr, nullptr, nullptr, nullptr);
}

int ansfm_layer_averageg(ansfm_ctx *ctx, int n_models, double RADIUS, int NPRO, const double *H, const double *P,
                         const double *T, int NVMR, const double *VMR, int NDUST, const double *DUST, const double *PARAH2,
                         int NLAY, const double *BASEH, double LAYANG, int LAYINT, double LAYHT, int NINT,
                         const int32_t *DUST_UNITS, const double *XMOLWT, double *HEIGHT, double *PRESS, double *TEMP,
                         double *TOTAM, double *AMOUNT, double *PP, double *CONT, double *FRAC, double *DELH, double *BASET,
                         double *LAYSF, double *DTE, double *DAM, double *DCO, double *DPH)
{
    return layer_average_impl(ctx, n_models, RADIUS, NPRO, H, P, T, NVMR, VMR, NDUST, DUST, PARAH2, NLAY, BASEH, LAYANG, LAYINT,
                              LAYHT, NINT, DUST_UNITS, XMOLWT, HEIGHT, PRESS, TEMP, TOTAM, AMOUNT, PP, CONT, FRAC, DELH, BASET,
                              LAYSF, true, DTE, DAM, DCO, DPH);
}

int ansfm_layer_average_dev(ansfm_ctx *ctx, int n_models, double RADIUS, int NPRO, const double *H, const double *P,
                            const double *T, int NVMR, const double *VMR, int NDUST, const double *DUST,
                            const double *PARAH2, int NLAY, const double *BASEH, double LAYANG, int LAYINT, double LAYHT,
                            int NINT, const int32_t *DUST_UNITS, const double *XMOLWT, double *out_dev)
{
    if (!out_dev) { CHECK_CTX(ctx); FAIL(ANSFM_ERR_INVALID, "layer_average_dev: bad argument"); }
    return layer_average_impl(ctx, n_models, RADIUS, NPRO, H, P, T, NVMR, VMR, NDUST, DUST, PARAH2, NLAY, BASEH, LAYANG, LAYINT,
                              LAYHT, NINT, DUST_UNITS, XMOLWT, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr, nullptr, nullptr, nullptr, false, nullptr, nullptr, nullptr, nullptr, out_dev);
}

}  // extern "C"
