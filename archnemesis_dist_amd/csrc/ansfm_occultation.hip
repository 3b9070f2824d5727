// ansfm_occultation.hip -- translation unit of the occultation kernels (ansfm_occultation_kernels.hip.h): the entry point
// ansfm_cirsradg_ck_occultation with the build of its compressed matrices and its launcher, and ansfm_occultation_last.  The gas
// stage it shares with the gradient RT entries and the transit entry is in ansfm_api.hip.  gfx950 only.
#include "ansfm_occultation_kernels.hip.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

// Slots of dk a chunk of k_occ_grad stages and the LDS of its block: the largest chunk that fits the two-block budget beside
// the waves' columns (the one-block budget where that holds no slot), then evened out over the chunks it takes; 0: no fit.
static int occ_chunk(int G, int NP1, size_t *lds_bytes)
{
    const size_t row = (size_t)G * kWave * sizeof(double), cols = kOccWaves * row;
    for (size_t budget : {kOccLdsTwoBlocks, kOccLdsOneBlock}) {
        if (budget < cols + row) continue;
        const int most = (int)std::min<size_t>((budget - cols) / row, (size_t)NP1);
        const int chunks = (NP1 + most - 1) / most, sc = (NP1 + chunks - 1) / chunks;
        *lds_bytes = cols + (size_t)sc * row;
        return sc;
    }
    return 0;
}

// k_occ_paths, then k_occ_grad, on ctx->stream, between the events occultation_last reads
static int launch_occultation(ansfm_ctx *ctx, const OccParams &q, size_t lds_grad)
{
    for (hipEvent_t &e : ctx->occ_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    const unsigned tiles = (unsigned)(q.Wpad / kWave);
    const size_t lds_paths = (size_t)q.L * kWave * sizeof(double);
    // more than the 64 KiB of dynamic LDS a kernel may have without the attribute
    if (lds_paths > (size_t)64 * 1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_occ_paths), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOccLdsOneBlock));
    if (lds_grad > (size_t)64 * 1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_occ_grad), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOccLdsOneBlock));
    HIPCHK(hipEventRecord(ctx->occ_ev[0], ctx->stream));
    hipLaunchKernelGGL(k_occ_paths, dim3(tiles, (unsigned)q.G), dim3(kWave), lds_paths, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->occ_ev[1], ctx->stream));
    hipLaunchKernelGGL(k_occ_grad, dim3(tiles, (unsigned)q.L), dim3(kOccWaves * kWave), lds_grad, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->occ_ev[2], ctx->stream));
    return ANSFM_OK;
}

// What the entry stages of the two matrices.  Sm[l][p] = sum of SCALE over the entries j < NLAYIN[p] of path p with
// LAYINC[j][p] = l (padding is never read), compressed by path; C as the caller gave it; C o Sm compressed by (layer, geometry)
// the way compress_path_matrix of the transit entry compresses Sm by layer: a pointer array over l Q + q, then the paths and the
// values C[q][p] Sm[l][p] in the order of geometry q's row.
//   hi = col_ptr [P + 1], col_lay [nnz], mix_ptr [Q + 1], mix_path [mnz], lq_ptr [L Q + 1], lq_path [lnz]
//   hd = col_val [nnz], mix_val [mnz], lq_val [lnz]
struct OccMatrices {
    std::vector<int32_t> hi;
    std::vector<double> hd;
    size_t nnz = 0, mnz = 0, lnz = 0;
};
static int compress_occultation(ansfm_ctx *ctx, int L, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                const double *SCALE, int Q, const int32_t *mix_ptr, const int32_t *mix_path, const double *mix_val,
                                OccMatrices &m)
{
    if (mix_ptr[0] != 0) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_occultation: mix_ptr[0] must be 0");
    for (int q = 0; q < Q; ++q)
        if (mix_ptr[q + 1] < mix_ptr[q]) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_occultation: mix_ptr must not decrease");
    const size_t mnz = (size_t)mix_ptr[Q];
    if (mnz && (!mix_path || !mix_val)) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_occultation: null mix_path / mix_val");
    for (size_t i = 0; i < mnz; ++i)
        if (mix_path[i] < 0 || mix_path[i] >= P) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_occultation: mix_path outside 0 .. P - 1");
    std::vector<double> Sm((size_t)L * P, 0.0);
    std::vector<char> hit((size_t)L * P, 0);
    for (int p = 0; p < P; ++p) {
        if (NLAYIN[p] < 0 || NLAYIN[p] > LIMAX) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_occultation: NLAYIN outside 0 .. LIMAX");
        for (int j = 0; j < NLAYIN[p]; ++j) {
            const int l = LAYINC[(size_t)j * P + p];
            if (l < 0 || l >= L) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_occultation: LAYINC outside 0 .. L - 1");
            Sm[(size_t)l * P + p] += SCALE[(size_t)j * P + p];
            hit[(size_t)l * P + p] = 1;
        }
    }
    size_t nnz = 0, lnz = 0;
    for (char h : hit) nnz += h;
    for (int l = 0; l < L; ++l)
        for (size_t i = 0; i < mnz; ++i) lnz += hit[(size_t)l * P + mix_path[i]];
    if (lnz > (size_t)INT32_MAX) FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_occultation: more than 2^31 - 1 (layer, geometry, path) entries");
    m.nnz = nnz; m.mnz = mnz; m.lnz = lnz;
    m.hi.assign((size_t)P + 1 + nnz + Q + 1 + mnz + (size_t)L * Q + 1 + lnz, 0);
    m.hd.assign(nnz + mnz + lnz, 0.0);
    int32_t *col_ptr = m.hi.data(), *col_lay = col_ptr + P + 1, *mp = col_lay + nnz, *mpath = mp + Q + 1, *lq_ptr = mpath + mnz,
            *lq_path = lq_ptr + (size_t)L * Q + 1;
    double *col_val = m.hd.data(), *mval = col_val + nnz, *lq_val = mval + mnz;
    int32_t n = 0;
    for (int p = 0; p < P; ++p) {
        col_ptr[p] = n;
        for (int l = 0; l < L; ++l)
            if (hit[(size_t)l * P + p]) { col_lay[n] = l; col_val[n++] = Sm[(size_t)l * P + p]; }
    }
    col_ptr[P] = n;
    std::copy(mix_ptr, mix_ptr + Q + 1, mp);
    std::copy(mix_path, mix_path + mnz, mpath);
    std::copy(mix_val, mix_val + mnz, mval);
    n = 0;
    for (int l = 0; l < L; ++l)
        for (int q = 0; q < Q; ++q) {
            lq_ptr[(size_t)l * Q + q] = n;
            for (int i = mix_ptr[q]; i < mix_ptr[q + 1]; ++i)
                if (hit[(size_t)l * P + mix_path[i]]) { lq_path[n] = mix_path[i]; lq_val[n++] = mix_val[i] * Sm[(size_t)l * P + mix_path[i]]; }
        }
    lq_ptr[(size_t)L * Q] = n;
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
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg_ck_occultation: upload a k-table first");
    if (L <= 0 || P <= 0 || LIMAX <= 0 || Q <= 0 || !lay_press_pa || !lay_temp || !amount || !NLAYIN || !LAYINC || !SCALE || !mix_ptr ||
        !MOD || !igas_map || NPAR <= 0 || NPAR > kMaxPar || NVMR < 0 || NVMR >= NPAR)
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_occultation: bad argument (NPAR <= 256)");
    if (L > kTransitMaxRows || P > kTransitMaxRows)
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_occultation: at most 320 layers and 320 paths (the 160 KiB LDS tile of k_occ_paths)");
    OccMatrices m;
    int rc;
    if ((rc = compress_occultation(ctx, L, P, LIMAX, NLAYIN, LAYINC, SCALE, Q, mix_ptr, mix_path, mix_val, m))) return rc;

    // everything that can refuse the arguments comes before the first copy is queued
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, S = ctx->S, NP1 = S + 1;
    const size_t D = sizeof(double);
    OccParams q;
    memset(&q, 0, sizeof q);
    q.gas_mask = ctx->is_lbl ? 0xFFFFFFFFu : ctx->grad_gas_mask;
    if ((rc = fill_slot_of_param(ctx, igas_map, NVMR, NPAR, q.gas_mask, q.slot_of_param))) return rc;
    size_t lds_grad = 0;
    if (!(q.SC = occ_chunk(G, NP1, &lds_grad)))
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_occultation: too many g-ordinates for the LDS of k_occ_grad");
    if (Wpad / kWave > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_occultation: more than 65535 wavenumber tiles (4.19e6 wavenumbers)");
    if (ctx->dcont_gas_L && ctx->dcont_gas_L != L) {
        ctx->dcont_gas_L = 0;
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_occultation: the pending shared gas gradient (ansfm_set_shared_gas_gradient) is for a "
                                "different number of layers");
    }
    HIPCHK(hipSetDevice(ctx->device));
    ctx->dspec_dims[0] = 0;
    ctx->occ_recorded = 0;
    // dMOD as a whole: 8 W NPAR L Q bytes.  A reservation that fails is the caller's cue to take the un-collapsed route.
    size_t n_dmod = 0;
    if (__builtin_mul_overflow((size_t)W * NPAR, (size_t)L * Q, &n_dmod) || n_dmod > SIZE_MAX / D ||
        ctx->dspec_ref.reserve(n_dmod * D) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_occultation: dMOD (8 W NPAR L Q bytes) could not be reserved on the device");
    }
    // m.hd / m.hi are staged from this frame: from here on no return before the stream has been synchronised
    auto on_device = [&]() -> int {
        Stager st{ctx};
        const double *press = st.up(lay_press_pa, L), *temp = st.up(lay_temp, L), *am = st.up(amount, (size_t)L * S),
                     *cont = st.up(taucont, (size_t)L * W), *dcont = st.up(dtaucon, (size_t)L * W * NPAR),
                     *dd = st.up(m.hd.data(), m.hd.size());
        const int32_t *di = st.up(m.hi.data(), m.hi.size());
        const double *xf = st.up(xfac, W);
        if (st.rc) return st.rc;
        int rc2;
        const double *cont_t = nullptr, *dcont_t = nullptr;
        if ((rc2 = grad_gas_stage(ctx, 1, L, press, temp, am, cont, dcont, NPAR, &cont_t, &dcont_t))) return rc2;
        // scratch beyond the gas stage: exp(-tau_path) [P][G][Wpad], MOD [W][Q], T [W][P]
        const size_t n_tpart = (size_t)P * G * Wpad, n_out = (size_t)W * ((size_t)Q + P);
        ctx->occ_scratch_bytes = (n_tpart + n_out) * D;
        HIPCHK(ctx->occ_ws.reserve(ctx->occ_scratch_bytes));
        q.tau = ctx->tau.as<double>();
        q.cont = cont_t;
        q.delg = ctx->d_delg.as<double>();
        q.xfac = xf;
        q.col_val = dd; q.mix_val = dd + m.nnz; q.lq_val = dd + m.nnz + m.mnz;
        q.col_ptr = di; q.col_lay = q.col_ptr + P + 1; q.mix_ptr = q.col_lay + m.nnz; q.mix_path = q.mix_ptr + Q + 1;
        q.lq_ptr = q.mix_path + m.mnz; q.lq_path = q.lq_ptr + (size_t)L * Q + 1;
        q.tpart = ctx->occ_ws.as<double>();
        q.mod = q.tpart + n_tpart;
        q.trans = q.mod + (size_t)W * Q;
        q.dmod = ctx->dspec_ref.as<double>();
        q.dk = ctx->dkbuf.as<double>();
        q.dcont = dcont_t;
        if (ctx->dcont_gas_L) {
            q.dcont_gas = ctx->dcont_gas.as<double>();
            ctx->dcont_gas_L = 0;               // one call only
        }
        q.W = W; q.Wpad = Wpad; q.G = G; q.L = L; q.P = P; q.Q = Q;
        q.NPAR = NPAR; q.NVMR = NVMR; q.NP1 = NP1;
        HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
        if ((rc2 = launch_occultation(ctx, q, lds_grad))) return rc2;
        HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
        call_recorded(ctx, 1, L);
        HIPCHK(hipMemcpyAsync(MOD, q.mod, (size_t)W * Q * D, hipMemcpyDeviceToHost, ctx->stream));
        if (TRANS) HIPCHK(hipMemcpyAsync(TRANS, q.trans, (size_t)W * P * D, hipMemcpyDeviceToHost, ctx->stream));
        if (dMOD) HIPCHK(hipMemcpyAsync(dMOD, q.dmod, n_dmod * D, hipMemcpyDeviceToHost, ctx->stream));
        return check_unsorted(ctx);             // synchronises
    };
    if ((rc = on_device())) {
        (void)hipStreamSynchronize(ctx->stream);   // whatever was queued from m.hd / m.hi has run before they go
        return rc;
    }
    ctx->dspec_dims[0] = W; ctx->dspec_dims[1] = NPAR; ctx->dspec_dims[2] = L; ctx->dspec_dims[3] = Q;
    ctx->occ_recorded = 1;
    return ANSFM_OK;
}

int ansfm_occultation_last(const ansfm_ctx *cctx, double info[3])
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);
    CHECK_CTX(ctx);
    if (!info) FAIL(ANSFM_ERR_INVALID, "occultation_last: null argument");
    if (!ctx->occ_recorded) FAIL(ANSFM_ERR_INVALID, "occultation_last: no ansfm_cirsradg_ck_occultation call recorded yet");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(ctx->occ_ev[2]));
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, ctx->occ_ev[0], ctx->occ_ev[1]));
    HIPCHK(hipEventElapsedTime(&b, ctx->occ_ev[1], ctx->occ_ev[2]));
    info[0] = (double)ctx->occ_scratch_bytes;
    info[1] = a;
    info[2] = b;
    return ANSFM_OK;
}

}  // extern "C"
