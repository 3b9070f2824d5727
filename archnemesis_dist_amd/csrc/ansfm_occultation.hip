// ansfm_occultation.hip -- translation unit of the occultation kernels (ansfm_occultation_kernels.hip.h): the entry point
// ansfm_cirsradg_ck_occultation with the build of its compressed matrices and its launcher, and ansfm_occultation_last.  The gas
// stage it shares with the gradient RT entries and the transit entry is in ansfm_api.hip.  gfx950 only.
#include "ansfm_occultation_kernels.hip.h"
#include "ansfm_pathmix.hip.h"

using namespace ansfm;

// k_occ_paths, then k_occ_grad, on ctx->stream, between the events occultation_last reads
static int launch_occultation(ansfm_ctx *ctx, const OccParams &q, size_t lds_grad)
{
    FusedRoute &r = ctx->occ;
    int rc;
    const unsigned tiles = (unsigned)(q.Wpad / kWave);
    const size_t lds_paths = (size_t)q.L * kWave * sizeof(double);
    if ((rc = ensure_events(ctx, r)) || (rc = allow_lds(ctx, k_occ_paths, lds_paths)) || (rc = allow_lds(ctx, k_occ_grad, lds_grad)))
        return rc;
    HIPCHK(hipEventRecord(r.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_occ_paths, dim3(tiles, (unsigned)q.G), dim3(kWave), lds_paths, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(r.ev[1], ctx->stream));
    hipLaunchKernelGGL(k_occ_grad, dim3(tiles, (unsigned)q.L), dim3(kMixWaves * kWave), lds_grad, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(r.ev[2], ctx->stream));
    return ANSFM_OK;
}

extern "C" {

// Solar occultation with gradients of one model (nemesisSOfmg, ForwardModel_0.py:983-1249), the tangent paths mixed to the Q
// geometries on the device: the gas stage of the gradient RT entries (grad_gas_stage), then k_occ_paths and k_occ_grad on the
// compressed matrices.  Neither trold_ws nor dspec_i nor the transit scratch is touched; dMOD (W, NPAR, L, Q) stays in dspec_ref
// for ansfm_map2pro(dSPECIN = NULL).
int ansfm_cirsradg_ck_occultation(ansfm_ctx *ctx, int L, const double *lay_press_pa, const double *lay_temp, const double *amount,
                                  const double *taucont, const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P,
                                  int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, int Q,
                                  const int32_t *mix_ptr, const int32_t *mix_path, const double *mix_val, const double *xfac,
                                  double *MOD, double *TRANS, double *dMOD)
{
    const char *what = "cirsradg_ck_occultation";
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg_ck_occultation: upload a k-table first");
    if (L <= 0 || P <= 0 || LIMAX <= 0 || Q <= 0 || !lay_press_pa || !lay_temp || !amount || !NLAYIN || !LAYINC || !SCALE || !mix_ptr ||
        !MOD || !igas_map || NPAR <= 0 || NPAR > kMaxPar || NVMR < 0 || NVMR >= NPAR)
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_occultation: bad argument (NPAR <= 256)");
    if (L > kTransitMaxRows || P > kTransitMaxRows)
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_occultation: at most 320 layers and 320 paths (the 160 KiB LDS tile of k_occ_paths)");
    int rc;
    size_t mnz = 0, lnz = 0;
    if ((rc = check_mix(ctx, what, P, Q, mix_ptr, mix_path, mix_val, &mnz)) || (rc = check_paths(ctx, what, L, P, LIMAX, NLAYIN, LAYINC)))
        return rc;
    // What is staged of the two matrices: Sm compressed by path; C as the caller gave it; C o Sm compressed by (layer, geometry):
    // a pointer array over l Q + q, then the paths and the values C[q][p] Sm[l][p] in the order of geometry q's row.
    //   hi = col_ptr [P + 1], col_lay [nnz], mix_ptr [Q + 1], mix_path [mnz], lq_ptr [L Q + 1], lq_path [lnz]
    //   hd = col_val [nnz], mix_val [mnz], lq_val [lnz]
    const PathMatrix m = build_path_matrix(L, P, NLAYIN, LAYINC, SCALE);
    const size_t nnz = m.nnz;
    for (int l = 0; l < L; ++l)
        for (size_t i = 0; i < mnz; ++i) lnz += m.hit[(size_t)l * P + mix_path[i]];
    if (lnz > (size_t)INT32_MAX) FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_occultation: more than 2^31 - 1 (layer, geometry, path) entries");
    std::vector<int32_t> hi(m.col_ptr), lq_path;
    hi.insert(hi.end(), m.col_lay.begin(), m.col_lay.end());
    hi.insert(hi.end(), mix_ptr, mix_ptr + Q + 1);
    hi.insert(hi.end(), mix_path, mix_path + mnz);
    std::vector<double> hd(m.col_val);
    hd.insert(hd.end(), mix_val, mix_val + mnz);
    for (int l = 0; l < L; ++l)
        for (int q = 0; q < Q; ++q) {
            hi.push_back((int32_t)lq_path.size());
            for (int i = mix_ptr[q]; i < mix_ptr[q + 1]; ++i)
                if (m.hit[(size_t)l * P + mix_path[i]]) {
                    lq_path.push_back(mix_path[i]);
                    hd.push_back(mix_val[i] * m.Sm[(size_t)l * P + mix_path[i]]);
                }
        }
    hi.push_back((int32_t)lq_path.size());
    hi.insert(hi.end(), lq_path.begin(), lq_path.end());

    // everything that can refuse the arguments comes before the first copy is queued
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, NP1 = ctx->S + 1;
    const size_t D = sizeof(double);
    OccParams q;
    size_t lds_grad = 0, n_dmod = 0;
    if ((rc = fused_prologue(ctx, what, ctx->occ, L, igas_map, NVMR, NPAR, q, "k_occ_grad", &q.SC, &lds_grad)) ||
        (rc = reserve_dmod(ctx, what, NPAR, L, Q, false, &n_dmod)))
        return rc;
    return fused_staged_call(
        ctx, ctx->occ, L, lay_press_pa, lay_temp, amount, taucont, dtaucon, NPAR, Q, hd, hi, xfac,
        [&](const FusedStaged &s, std::vector<FusedCopy> &copies) -> int {
            // scratch beyond the gas stage: exp(-tau_path) [P][G][Wpad], MOD [W][Q], T [W][P]
            const size_t n_tpart = (size_t)P * G * Wpad, n_out = (size_t)W * ((size_t)Q + P);
            ctx->occ.scratch_bytes = (n_tpart + n_out) * D;
            HIPCHK(ctx->occ.ws.reserve(ctx->occ.scratch_bytes));
            q.tau = ctx->tau.as<double>();
            q.cont = s.cont_t;
            q.delg = ctx->d_delg.as<double>();
            q.xfac = s.xfac;
            q.col_val = s.dd; q.mix_val = s.dd + nnz; q.lq_val = s.dd + nnz + mnz;
            q.col_ptr = s.di; q.col_lay = q.col_ptr + P + 1; q.mix_ptr = q.col_lay + nnz; q.mix_path = q.mix_ptr + Q + 1;
            q.lq_ptr = q.mix_path + mnz; q.lq_path = q.lq_ptr + (size_t)L * Q + 1;
            q.tpart = ctx->occ.ws.as<double>();
            q.mod = q.tpart + n_tpart;
            q.trans = q.mod + (size_t)W * Q;
            q.dmod = ctx->dspec_ref.as<double>();
            q.dk = ctx->dkbuf.as<double>();
            q.dcont = s.dcont_t;
            q.dcont_gas = s.dcont_gas;
            q.W = W; q.Wpad = Wpad; q.G = G; q.L = L; q.P = P; q.Q = Q;
            q.NPAR = NPAR; q.NVMR = NVMR; q.NP1 = NP1;
            copies = {{MOD, q.mod, (size_t)W * Q * D}, {TRANS, q.trans, (size_t)W * P * D}, {dMOD, q.dmod, n_dmod * D}};
            return ANSFM_OK;
        },
        [&]() { return launch_occultation(ctx, q, lds_grad); });
}

int ansfm_occultation_last(const ansfm_ctx *ctx, double info[3]) { return fused_last(ctx, &ansfm_ctx::occ, info, "occultation"); }

}  // extern "C"
