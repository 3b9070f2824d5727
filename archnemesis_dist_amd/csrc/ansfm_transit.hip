// ansfm_transit.hip -- translation unit of the transit kernels (ansfm_transit_kernels.hip.h): the entry point
// ansfm_cirsradg_ck_transit with its path-matrix build and its launcher, and ansfm_transit_last.  The gas stage it shares with
// the gradient RT entries is in ansfm_api.hip.  gfx950 only.
#include "ansfm_transit_kernels.hip.h"
#include "ansfm_pathmix.hip.h"

using namespace ansfm;

// k_transit_sens, then k_transit_grad, on ctx->stream, between the events transit_last reads
static int launch_transit(ansfm_ctx *ctx, const TransitParams &q)
{
    const int rows = std::max(q.L, q.P);
    if (rows > kTransitMaxRows) FAIL(ANSFM_ERR_UNSUPPORTED, "transit: more than 320 layers or paths (the 160 KiB LDS tile of k_transit_sens)");
    if (q.Wpad / kWave > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "transit: more than 65535 wavenumber tiles (4.19e6 wavenumbers)");
    FusedRoute &r = ctx->transit;
    int rc;
    const unsigned tiles = (unsigned)(q.Wpad / kWave);
    const size_t lds_sens = (size_t)rows * kWave * sizeof(double);
    if ((rc = ensure_events(ctx, r)) || (rc = allow_lds(ctx, k_transit_sens, lds_sens))) return rc;
    HIPCHK(hipEventRecord(r.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_transit_sens, dim3(tiles, (unsigned)q.G), dim3(kWave), lds_sens, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(r.ev[1], ctx->stream));
    hipLaunchKernelGGL(k_transit_grad, dim3(tiles, (unsigned)rows), dim3(kWave), (size_t)(q.G + q.NP1) * kWave * sizeof(double),
                       ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(r.ev[2], ctx->stream));
    return ANSFM_OK;
}

extern "C" {

// Primary-transit depth with gradients of one model (nemesisPTfm, ForwardModel_0.py:1838-1995), collapsed over the paths on the
// device: the gas stage of the gradient RT entries (grad_gas_stage), then k_transit_sens and k_transit_grad on the path matrix
// compressed by path and by layer.  Neither trold_ws nor dspec_i is reserved; dAREA (W, NPAR, L, 1) stays in dspec_ref for
// ansfm_map2pro(dSPECIN = NULL).
int ansfm_cirsradg_ck_transit(ansfm_ctx *ctx, int L, const double *lay_press_pa, const double *lay_temp, const double *amount,
                              const double *taucont, const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P,
                              int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                              const double *path_weight, double *AREA, double *TRANS, double *dAREA)
{
    const char *what = "cirsradg_ck_transit";
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg_ck_transit: upload a k-table first");
    if (L <= 0 || P <= 0 || LIMAX <= 0 || !lay_press_pa || !lay_temp || !amount || !NLAYIN || !LAYINC || !SCALE || !path_weight ||
        !AREA || !igas_map || NPAR <= 0 || NPAR > kMaxPar || NVMR < 0 || NVMR >= NPAR)
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_transit: bad argument (NPAR <= 256)");
    if (L > kTransitMaxRows || P > kTransitMaxRows)
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_transit: at most 320 layers and 320 paths (the 160 KiB LDS tile of k_transit_sens)");
    int rc;
    if ((rc = check_paths(ctx, what, L, P, LIMAX, NLAYIN, LAYINC))) return rc;
    // what is staged: hi = col_ptr [P + 1], col_lay [nnz], row_ptr [L + 1], row_path [nnz]; hd = path_weight [P], col_val [nnz],
    // row_val [nnz], the rows being Sm compressed by layer
    const PathMatrix m = build_path_matrix(L, P, NLAYIN, LAYINC, SCALE);
    const size_t nnz = m.nnz;
    std::vector<int32_t> hi(m.col_ptr);
    hi.insert(hi.end(), m.col_lay.begin(), m.col_lay.end());
    std::vector<double> hd(path_weight, path_weight + P), row_val;
    hd.insert(hd.end(), m.col_val.begin(), m.col_val.end());
    std::vector<int32_t> row_path;
    for (int l = 0; l < L; ++l) {
        hi.push_back((int32_t)row_path.size());
        for (int p = 0; p < P; ++p)
            if (m.hit[(size_t)l * P + p]) { row_path.push_back(p); row_val.push_back(m.Sm[(size_t)l * P + p]); }
    }
    hi.push_back((int32_t)row_path.size());
    hi.insert(hi.end(), row_path.begin(), row_path.end());
    hd.insert(hd.end(), row_val.begin(), row_val.end());

    // everything that can refuse the arguments comes before the first copy is queued
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, NP1 = ctx->S + 1;
    const size_t D = sizeof(double);
    TransitParams q;
    if ((rc = fused_prologue(ctx, what, ctx->transit, L, igas_map, NVMR, NPAR, q))) return rc;
    return fused_staged_call(
        ctx, ctx->transit, L, lay_press_pa, lay_temp, amount, taucont, dtaucon, NPAR, 1, hd, hi, nullptr,
        [&](const FusedStaged &s, std::vector<FusedCopy> &copies) -> int {
            // scratch beyond the gas stage: A [L][G][Wpad], exp(-tau_path) [P][G][Wpad], AREA [W], T [W][P]
            const size_t n_sens = (size_t)L * G * Wpad, n_tpart = (size_t)P * G * Wpad, n_out = (size_t)W * (1 + P);
            ctx->transit.scratch_bytes = (n_sens + n_tpart + n_out) * D;
            HIPCHK(ctx->transit.ws.reserve(ctx->transit.scratch_bytes));
            HIPCHK(ctx->dspec_ref.reserve((size_t)W * NPAR * L * D));
            q.tau = ctx->tau.as<double>();
            q.cont = s.cont_t;
            q.delg = ctx->d_delg.as<double>();
            q.weight = s.dd; q.col_val = s.dd + P; q.row_val = s.dd + P + nnz;
            q.col_ptr = s.di; q.col_lay = s.di + P + 1; q.row_ptr = s.di + P + 1 + nnz; q.row_path = s.di + P + 1 + nnz + L + 1;
            q.sens = ctx->transit.ws.as<double>();
            q.tpart = q.sens + n_sens;
            q.area = q.tpart + n_tpart;
            q.trans = q.area + W;
            q.darea = ctx->dspec_ref.as<double>();
            q.dk = ctx->dkbuf.as<double>();
            q.dcont = s.dcont_t;
            q.dcont_gas = s.dcont_gas;
            q.W = W; q.Wpad = Wpad; q.G = G; q.L = L; q.P = P;
            q.NPAR = NPAR; q.NVMR = NVMR; q.NP1 = NP1;
            copies = {{AREA, q.area, (size_t)W * D}, {TRANS, q.trans, (size_t)W * P * D}, {dAREA, q.darea, (size_t)W * NPAR * L * D}};
            return ANSFM_OK;
        },
        [&]() { return launch_transit(ctx, q); });
}

int ansfm_transit_last(const ansfm_ctx *ctx, double info[3]) { return fused_last(ctx, &ansfm_ctx::transit, info, "transit"); }

}  // extern "C"
