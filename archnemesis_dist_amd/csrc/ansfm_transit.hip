// ansfm_transit.hip -- translation unit of the transit kernels (ansfm_transit_kernels.hip.h): the entry point
// ansfm_cirsradg_ck_transit with its path-matrix build and its launcher, and ansfm_transit_last.  The gas stage it shares with
// the gradient RT entries is in ansfm_api.hip.  gfx950 only.
#include "ansfm_transit_kernels.hip.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

// k_transit_sens, then k_transit_grad, on ctx->stream, between the events transit_last reads
static int launch_transit(ansfm_ctx *ctx, const TransitParams &q)
{
    const int rows = std::max(q.L, q.P);
    if (rows > kTransitMaxRows) FAIL(ANSFM_ERR_UNSUPPORTED, "transit: more than 320 layers or paths (the 160 KiB LDS tile of k_transit_sens)");
    if (q.Wpad / kWave > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "transit: more than 65535 wavenumber tiles (4.19e6 wavenumbers)");
    for (hipEvent_t &e : ctx->transit_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    const unsigned tiles = (unsigned)(q.Wpad / kWave);
    HIPCHK(hipEventRecord(ctx->transit_ev[0], ctx->stream));
    hipLaunchKernelGGL(k_transit_sens, dim3(tiles, (unsigned)q.G), dim3(kWave), (size_t)rows * kWave * sizeof(double), ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->transit_ev[1], ctx->stream));
    hipLaunchKernelGGL(k_transit_grad, dim3(tiles, (unsigned)rows), dim3(kWave), (size_t)(q.G + q.NP1) * kWave * sizeof(double),
                       ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->transit_ev[2], ctx->stream));
    return ANSFM_OK;
}

// The path matrix Sm[l][p] = sum of SCALE over the entries j < NLAYIN[p] of path p with LAYINC[j][p] = l, compressed by path
// and by layer; an entry is what some j < NLAYIN[p] touched, padding is never read.  The two host vectors are what the entry
// stages: hi = col_ptr [P + 1], col_lay [nnz], row_ptr [L + 1], row_path [nnz]; hd = path_weight [P], col_val [nnz], row_val [nnz].
static int compress_path_matrix(ansfm_ctx *ctx, int L, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                const double *SCALE, const double *path_weight, std::vector<int32_t> &hi, std::vector<double> &hd,
                                size_t *nnz_out)
{
    std::vector<double> Sm((size_t)L * P, 0.0);
    std::vector<char> hit((size_t)L * P, 0);
    for (int p = 0; p < P; ++p) {
        if (NLAYIN[p] < 0 || NLAYIN[p] > LIMAX) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_transit: NLAYIN outside 0 .. LIMAX");
        for (int j = 0; j < NLAYIN[p]; ++j) {
            const int l = LAYINC[(size_t)j * P + p];
            if (l < 0 || l >= L) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_transit: LAYINC outside 0 .. L - 1");
            Sm[(size_t)l * P + p] += SCALE[(size_t)j * P + p];
            hit[(size_t)l * P + p] = 1;
        }
    }
    size_t nnz = 0;
    for (char h : hit) nnz += h;
    hi.assign((size_t)P + 1 + L + 1 + 2 * nnz, 0);
    hd.assign((size_t)P + 2 * nnz, 0.0);
    int32_t *col_ptr = hi.data(), *col_lay = col_ptr + P + 1, *row_ptr = col_lay + nnz, *row_path = row_ptr + L + 1;
    double *col_val = hd.data() + P, *row_val = col_val + nnz;
    std::copy(path_weight, path_weight + P, hd.data());
    int32_t n = 0;
    for (int p = 0; p < P; ++p) {
        col_ptr[p] = n;
        for (int l = 0; l < L; ++l)
            if (hit[(size_t)l * P + p]) { col_lay[n] = l; col_val[n++] = Sm[(size_t)l * P + p]; }
    }
    col_ptr[P] = n;
    n = 0;
    for (int l = 0; l < L; ++l) {
        row_ptr[l] = n;
        for (int p = 0; p < P; ++p)
            if (hit[(size_t)l * P + p]) { row_path[n] = p; row_val[n++] = Sm[(size_t)l * P + p]; }
    }
    row_ptr[L] = n;
    *nnz_out = nnz;
    return ANSFM_OK;
}

extern "C" {

// Primary-transit depth with gradients of one model (nemesisPTfm, ForwardModel_0.py:1838-1995), collapsed over the paths on the
// device: the gas stage of the gradient RT entries (grad_gas_stage), then k_transit_sens and k_transit_grad on the compressed
// path matrix.  Neither trold_ws nor dspec_i is reserved; dAREA (W, NPAR, L, 1) stays in dspec_ref for
// ansfm_map2pro(dSPECIN = NULL).
int ansfm_cirsradg_ck_transit(ansfm_ctx *ctx, int L, const double *lay_press_pa, const double *lay_temp, const double *amount,
                              const double *taucont, const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P,
                              int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                              const double *path_weight, double *AREA, double *TRANS, double *dAREA)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg_ck_transit: upload a k-table first");
    if (L <= 0 || P <= 0 || LIMAX <= 0 || !lay_press_pa || !lay_temp || !amount || !NLAYIN || !LAYINC || !SCALE || !path_weight ||
        !AREA || !igas_map || NPAR <= 0 || NPAR > kMaxPar || NVMR < 0 || NVMR >= NPAR)
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_transit: bad argument (NPAR <= 256)");
    if (L > kTransitMaxRows || P > kTransitMaxRows)
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_transit: at most 320 layers and 320 paths (the 160 KiB LDS tile of k_transit_sens)");
    std::vector<int32_t> hi;
    std::vector<double> hd;
    size_t nnz = 0;
    int rc;
    if ((rc = compress_path_matrix(ctx, L, P, LIMAX, NLAYIN, LAYINC, SCALE, path_weight, hi, hd, &nnz))) return rc;

    // everything that can refuse the arguments comes before the first copy is queued
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, S = ctx->S, NP1 = S + 1;
    const size_t D = sizeof(double);
    TransitParams q;
    memset(&q, 0, sizeof q);
    q.gas_mask = ctx->is_lbl ? 0xFFFFFFFFu : ctx->grad_gas_mask;
    if ((rc = fill_slot_of_param(ctx, igas_map, NVMR, NPAR, q.gas_mask, q.slot_of_param))) return rc;
    if (ctx->dcont_gas_L && ctx->dcont_gas_L != L) {
        ctx->dcont_gas_L = 0;
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_transit: the pending shared gas gradient (ansfm_set_shared_gas_gradient) is for a "
                                "different number of layers");
    }
    HIPCHK(hipSetDevice(ctx->device));
    ctx->dspec_dims[0] = 0;
    ctx->transit_recorded = 0;
    // hd / hi are staged from this frame: from here on no return before the stream has been synchronised
    auto on_device = [&]() -> int {
        Stager st{ctx};
        const double *press = st.up(lay_press_pa, L), *temp = st.up(lay_temp, L), *am = st.up(amount, (size_t)L * S),
                     *cont = st.up(taucont, (size_t)L * W), *dcont = st.up(dtaucon, (size_t)L * W * NPAR),
                     *dd = st.up(hd.data(), hd.size());
        const int32_t *di = st.up(hi.data(), hi.size());
        if (st.rc) return st.rc;
        int rc2;
        const double *cont_t = nullptr, *dcont_t = nullptr;
        if ((rc2 = grad_gas_stage(ctx, 1, L, press, temp, am, cont, dcont, NPAR, &cont_t, &dcont_t))) return rc2;
        // scratch beyond the gas stage: A [L][G][Wpad], exp(-tau_path) [P][G][Wpad], AREA [W], T [W][P]
        const size_t n_sens = (size_t)L * G * Wpad, n_tpart = (size_t)P * G * Wpad, n_out = (size_t)W * (1 + P);
        ctx->transit_scratch_bytes = (n_sens + n_tpart + n_out) * D;
        HIPCHK(ctx->transit_ws.reserve(ctx->transit_scratch_bytes));
        HIPCHK(ctx->dspec_ref.reserve((size_t)W * NPAR * L * D));
        q.tau = ctx->tau.as<double>();
        q.cont = cont_t;
        q.delg = ctx->d_delg.as<double>();
        q.weight = dd; q.col_val = dd + P; q.row_val = dd + P + nnz;
        q.col_ptr = di; q.col_lay = di + P + 1; q.row_ptr = di + P + 1 + nnz; q.row_path = di + P + 1 + nnz + L + 1;
        q.sens = ctx->transit_ws.as<double>();
        q.tpart = q.sens + n_sens;
        q.area = q.tpart + n_tpart;
        q.trans = q.area + W;
        q.darea = ctx->dspec_ref.as<double>();
        q.dk = ctx->dkbuf.as<double>();
        q.dcont = dcont_t;
        if (ctx->dcont_gas_L) {
            q.dcont_gas = ctx->dcont_gas.as<double>();
            ctx->dcont_gas_L = 0;               // one call only
        }
        q.W = W; q.Wpad = Wpad; q.G = G; q.L = L; q.P = P;
        q.NPAR = NPAR; q.NVMR = NVMR; q.NP1 = NP1;
        HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
        if ((rc2 = launch_transit(ctx, q))) return rc2;
        HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
        call_recorded(ctx, 1, L);
        HIPCHK(hipMemcpyAsync(AREA, q.area, (size_t)W * D, hipMemcpyDeviceToHost, ctx->stream));
        if (TRANS) HIPCHK(hipMemcpyAsync(TRANS, q.trans, (size_t)W * P * D, hipMemcpyDeviceToHost, ctx->stream));
        if (dAREA) HIPCHK(hipMemcpyAsync(dAREA, q.darea, (size_t)W * NPAR * L * D, hipMemcpyDeviceToHost, ctx->stream));
        return check_unsorted(ctx);             // synchronises
    };
    if ((rc = on_device())) {
        (void)hipStreamSynchronize(ctx->stream);   // whatever was queued from hd / hi has run before they go
        return rc;
    }
    ctx->dspec_dims[0] = W; ctx->dspec_dims[1] = NPAR; ctx->dspec_dims[2] = L; ctx->dspec_dims[3] = 1;
    ctx->transit_recorded = 1;
    return ANSFM_OK;
}

int ansfm_transit_last(const ansfm_ctx *cctx, double info[3])
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);
    CHECK_CTX(ctx);
    if (!info) FAIL(ANSFM_ERR_INVALID, "transit_last: null argument");
    if (!ctx->transit_recorded) FAIL(ANSFM_ERR_INVALID, "transit_last: no ansfm_cirsradg_ck_transit call recorded yet");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(ctx->transit_ev[2]));
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, ctx->transit_ev[0], ctx->transit_ev[1]));
    HIPCHK(hipEventElapsedTime(&b, ctx->transit_ev[1], ctx->transit_ev[2]));
    info[0] = (double)ctx->transit_scratch_bytes;
    info[1] = a;
    info[2] = b;
    return ANSFM_OK;
}

}  // extern "C"
