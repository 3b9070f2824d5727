// ansfm_limb.hip -- translation unit of the limb-emission kernels (ansfm_limb_kernels.hip.h): the entry point
// ansfm_cirsradg_ck_limb with the build of its index arrays and its launcher, and ansfm_limb_last.  The gas stage it shares with
// the gradient RT entries, the transit entry and the occultation entry is in ansfm_api.hip.  gfx950 only.
#include "ansfm_limb_kernels.hip.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

// Slots of dk a chunk of k_limb_grad stages and the LDS of its block: the largest chunk that fits the two-block budget beside
// the waves' columns (the one-block budget where that holds no slot), then evened out over the chunks it takes; 0: no fit.
static int limb_chunk(int G, int NP1, size_t *lds_bytes)
{
    const size_t row = (size_t)G * kWave * sizeof(double), cols = kLimbWaves * row;
    for (size_t budget : {kLimbLdsTwoBlocks, kLimbLdsOneBlock}) {
        if (budget < cols + row) continue;
        const int most = (int)std::min<size_t>((budget - cols) / row, (size_t)NP1);
        const int chunks = (NP1 + most - 1) / most, sc = (NP1 + chunks - 1) / chunks;
        *lds_bytes = cols + (size_t)sc * row;
        return sc;
    }
    return 0;
}

// k_limb_planck and k_limb_sens, then k_limb_grad, on ctx->stream, between the events limb_last reads
static int launch_limb(ansfm_ctx *ctx, const LimbParams &q, size_t lds_grad)
{
    for (hipEvent_t &e : ctx->limb_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    const unsigned tiles = (unsigned)(q.Wpad / kWave);
    const size_t lds_sens = (size_t)2 * q.L * kWave * sizeof(double);
    // more than the 64 KiB of dynamic LDS a kernel may have without the attribute
    if (lds_sens > (size_t)64 * 1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_limb_sens), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLimbLdsOneBlock));
    if (lds_grad > (size_t)64 * 1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_limb_grad), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLimbLdsOneBlock));
    HIPCHK(hipEventRecord(ctx->limb_ev[0], ctx->stream));
    if (q.NT) {
        hipLaunchKernelGGL(k_limb_planck, dim3(tiles, (unsigned)q.NT), dim3(kWave), 0, ctx->stream, q);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_limb_sens, dim3(tiles, (unsigned)(q.Q + (q.n_orphan ? 1 : 0)), (unsigned)q.GS), dim3(kWave), lds_sens, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->limb_ev[1], ctx->stream));
    hipLaunchKernelGGL(k_limb_grad, dim3(tiles, (unsigned)q.L), dim3(kLimbWaves * kWave), lds_grad, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->limb_ev[2], ctx->stream));
    return ANSFM_OK;
}

// What the entry stages of the paths and the mix, after checking them.
//   hi = NLAYIN [P], LAYINC [LIMAX P] (padding entries 0), tidx [LIMAX P], mix_ptr [Q + 1], mix_path [mnz], mix_first [mnz],
//        orphan [n_orphan], hit [L Q]
//   hd = SCALE [LIMAX P], the distinct EMTEMP values [NT] (distinct as bit patterns, in the order of their first entry, path by
//        path), mix_val [mnz]
struct LimbArrays {
    std::vector<int32_t> hi;
    std::vector<double> hd;
    size_t mnz = 0, n_orphan = 0, NT = 0;
};
static int stage_limb(ansfm_ctx *ctx, int L, const double *lay_press_pa, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                      const double *SCALE, const double *EMTEMP, int Q, const int32_t *mix_ptr, const int32_t *mix_path,
                      const double *mix_val, LimbArrays &m)
{
    if (mix_ptr[0] != 0) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_limb: mix_ptr[0] must be 0");
    for (int q = 0; q < Q; ++q)
        if (mix_ptr[q + 1] < mix_ptr[q]) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_limb: mix_ptr must not decrease");
    const size_t mnz = (size_t)mix_ptr[Q], LP = (size_t)LIMAX * P;
    if (mnz && (!mix_path || !mix_val)) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_limb: null mix_path / mix_val");
    for (size_t i = 0; i < mnz; ++i)
        if (mix_path[i] < 0 || mix_path[i] >= P) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_limb: mix_path outside 0 .. P - 1");
    for (int p = 0; p < P; ++p) {
        if (NLAYIN[p] < 0 || NLAYIN[p] > LIMAX) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_limb: NLAYIN outside 0 .. LIMAX");
        for (int j = 0; j < NLAYIN[p]; ++j)
            if (LAYINC[(size_t)j * P + p] < 0 || LAYINC[(size_t)j * P + p] >= L)
                FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_limb: LAYINC outside 0 .. L - 1");
    }
    // the test of :6479-6483 as k_thermal_rtg makes it: a path whose last layer lies deeper than its middle one ends at the ground
    for (int p = 0; p < P; ++p) {
        const int nl = NLAYIN[p];
        if (!nl) continue;
        int i1 = (int)(nl / 2.0) - 1;
        if (i1 < 0) i1 += nl;
        if (lay_press_pa[LAYINC[(size_t)(nl - 1) * P + p]] > lay_press_pa[LAYINC[(size_t)i1 * P + p]])
            FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_limb: a path ends at the lower boundary (limb paths only; the surface term is not "
                                        "part of the fused call)");
    }
    std::vector<char> named(P, 0);
    std::vector<int32_t> first(mnz, 0), orphan;
    for (size_t i = 0; i < mnz; ++i)
        if (!named[mix_path[i]]) { named[mix_path[i]] = 1; first[i] = 1; }
    for (int p = 0; p < P; ++p)
        if (!named[p]) orphan.push_back(p);
    std::map<uint64_t, int32_t> seen;
    std::vector<double> tvals;
    std::vector<int32_t> tidx(LP, 0), lay(LP, 0);
    for (int p = 0; p < P; ++p)
        for (int j = 0; j < NLAYIN[p]; ++j) {
            const size_t e = (size_t)j * P + p;
            uint64_t bits;
            memcpy(&bits, &EMTEMP[e], sizeof bits);
            auto it = seen.find(bits);
            if (it == seen.end()) {
                it = seen.emplace(bits, (int32_t)tvals.size()).first;
                tvals.push_back(EMTEMP[e]);
            }
            tidx[e] = it->second;
            lay[e] = LAYINC[e];
        }
    if (tvals.size() > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_limb: more than 65535 distinct EMTEMP values");
    std::vector<int32_t> hit((size_t)L * Q, 0);
    for (int q = 0; q < Q; ++q)
        for (int i = mix_ptr[q]; i < mix_ptr[q + 1]; ++i) {
            const int p = mix_path[i];
            for (int j = 0; j < NLAYIN[p]; ++j) hit[(size_t)LAYINC[(size_t)j * P + p] * Q + q] = 1;
        }
    m.mnz = mnz; m.n_orphan = orphan.size(); m.NT = tvals.size();
    m.hi.clear();
    m.hi.insert(m.hi.end(), NLAYIN, NLAYIN + P);
    m.hi.insert(m.hi.end(), lay.begin(), lay.end());
    m.hi.insert(m.hi.end(), tidx.begin(), tidx.end());
    m.hi.insert(m.hi.end(), mix_ptr, mix_ptr + Q + 1);
    m.hi.insert(m.hi.end(), mix_path, mix_path + mnz);
    m.hi.insert(m.hi.end(), first.begin(), first.end());
    m.hi.insert(m.hi.end(), orphan.begin(), orphan.end());
    m.hi.insert(m.hi.end(), hit.begin(), hit.end());
    m.hd.assign(SCALE, SCALE + LP);
    m.hd.insert(m.hd.end(), tvals.begin(), tvals.end());
    m.hd.insert(m.hd.end(), mix_val, mix_val + mnz);
    return ANSFM_OK;
}

extern "C" {

// Limb thermal emission with gradients of one model (nemesisLfmg, ForwardModel_0.py:1372-1521), the tangent paths mixed to the Q
// geometries on the device: the gas stage of the gradient RT entries (grad_gas_stage), then k_limb_planck, k_limb_sens and
// k_limb_grad.  Neither trold_ws nor dspec_i nor the scratch of the transit or occultation entry is touched; dMOD
// (W, NPAR, L, Q) stays in dspec_ref for ansfm_map2pro(dSPECIN = NULL).
int ansfm_cirsradg_ck_limb(ansfm_ctx *ctx, int ISPACE, int L, const double *lay_press_pa, const double *lay_temp, const double *amount,
                           const double *taucont, const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P, int LIMAX,
                           const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, const double *EMTEMP, int Q,
                           const int32_t *mix_ptr, const int32_t *mix_path, const double *mix_val, const double *xfac, double *MOD,
                           double *SPEC, double *dMOD)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg_ck_limb: upload a k-table first");
    if (L <= 0 || P <= 0 || LIMAX <= 0 || Q <= 0 || !lay_press_pa || !lay_temp || !amount || !NLAYIN || !LAYINC || !SCALE || !EMTEMP ||
        !mix_ptr || !MOD || !igas_map || NPAR <= 0 || NPAR > kMaxPar || NVMR < 0 || NVMR >= NPAR || (ISPACE != 0 && ISPACE != 1))
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_limb: bad argument (NPAR <= 256, ISPACE 0 or 1)");
    if (L > kLimbMaxLayers)
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_limb: at most 160 layers (the two 64-lane LDS rows per layer of k_limb_sens, 160 KiB)");
    if (Q > 65534) FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_limb: more than 65534 geometries");
    LimbArrays m;
    int rc;
    if ((rc = stage_limb(ctx, L, lay_press_pa, P, LIMAX, NLAYIN, LAYINC, SCALE, EMTEMP, Q, mix_ptr, mix_path, mix_val, m))) return rc;

    // everything that can refuse the arguments comes before the first copy is queued
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, S = ctx->S, NP1 = S + 1;
    const size_t D = sizeof(double);
    LimbParams q;
    memset(&q, 0, sizeof q);
    q.gas_mask = ctx->is_lbl ? 0xFFFFFFFFu : ctx->grad_gas_mask;
    if ((rc = fill_slot_of_param(ctx, igas_map, NVMR, NPAR, q.gas_mask, q.slot_of_param))) return rc;
    size_t lds_grad = 0;
    if (!(q.SC = limb_chunk(G, NP1, &lds_grad)))
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_limb: too many g-ordinates for the LDS of k_limb_grad");
    if (Wpad / kWave > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_limb: more than 65535 wavenumber tiles (4.19e6 wavenumbers)");
    if (ctx->dcont_gas_L && ctx->dcont_gas_L != L) {
        ctx->dcont_gas_L = 0;
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_limb: the pending shared gas gradient (ansfm_set_shared_gas_gradient) is for a "
                                "different number of layers");
    }
    HIPCHK(hipSetDevice(ctx->device));
    ctx->dspec_dims[0] = 0;
    ctx->limb_recorded = 0;
    // dMOD as a whole, 8 W NPAR L Q bytes, and the scratch beyond the gas stage: B and dB/dT [NT][Wpad] each, spec [P][G][Wpad],
    // dg E [Q][L][G][Wpad], the partial sums of Z [GS][Q][L][Wpad], MOD [W][Q], SPEC [W][P].  A reservation that fails is the
    // caller's cue to take the un-collapsed route.
    const int GS = std::min(G, kLimbGroups);
    const size_t n_tab = m.NT * (size_t)Wpad, n_spec = (size_t)P * G * Wpad, n_out = (size_t)W * ((size_t)Q + P);
    size_t n_dmod = 0, n_E = 0, n_Z = 0;
    if (__builtin_mul_overflow((size_t)W * NPAR, (size_t)L * Q, &n_dmod) || n_dmod > SIZE_MAX / D ||
        __builtin_mul_overflow((size_t)Q * L, (size_t)G * Wpad, &n_E) || n_E > SIZE_MAX / (4 * D) ||
        ctx->dspec_ref.reserve(n_dmod * D) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_limb: dMOD (8 W NPAR L Q bytes) could not be reserved on the device");
    }
    n_Z = (size_t)GS * Q * L * Wpad;
    const size_t scratch = (2 * n_tab + n_spec + n_E + n_Z + n_out) * D;
    if (ctx->limb_ws.reserve(scratch) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_limb: the scratch (8 Q L G Wpad bytes and smaller arrays) could not be reserved on the device");
    }
    ctx->limb_scratch_bytes = scratch;
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
        const size_t LP = (size_t)LIMAX * P;
        q.tau = ctx->tau.as<double>();
        q.cont = cont_t;
        q.delg = ctx->d_delg.as<double>();
        q.xfac = xf;
        q.wave = ctx->d_wave.as<double>();
        q.nlayin = di; q.layinc = q.nlayin + P; q.tidx = q.layinc + LP; q.mix_ptr = q.tidx + LP; q.mix_path = q.mix_ptr + Q + 1;
        q.mix_first = q.mix_path + m.mnz; q.orphan = q.mix_first + m.mnz; q.hit = q.orphan + m.n_orphan;
        q.scale = dd; q.tvals = dd + LP; q.mix_val = q.tvals + m.NT;
        q.btab = ctx->limb_ws.as<double>();
        q.dbtab = q.btab + n_tab;
        q.spec = q.dbtab + n_tab;
        q.E = q.spec + n_spec;
        q.Zp = q.E + n_E;
        q.mod = q.Zp + n_Z;
        q.specout = q.mod + (size_t)W * Q;
        q.dmod = ctx->dspec_ref.as<double>();
        q.dk = ctx->dkbuf.as<double>();
        q.dcont = dcont_t;
        if (ctx->dcont_gas_L) {
            q.dcont_gas = ctx->dcont_gas.as<double>();
            ctx->dcont_gas_L = 0;               // one call only
        }
        q.W = W; q.Wpad = Wpad; q.G = G; q.L = L; q.P = P; q.Q = Q;
        q.GS = GS; q.NT = (int)m.NT; q.n_orphan = (int)m.n_orphan; q.ispace = ISPACE;
        q.NPAR = NPAR; q.NVMR = NVMR; q.NP1 = NP1;
        HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
        if ((rc2 = launch_limb(ctx, q, lds_grad))) return rc2;
        HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
        call_recorded(ctx, 1, L);
        HIPCHK(hipMemcpyAsync(MOD, q.mod, (size_t)W * Q * D, hipMemcpyDeviceToHost, ctx->stream));
        if (SPEC) HIPCHK(hipMemcpyAsync(SPEC, q.specout, (size_t)W * P * D, hipMemcpyDeviceToHost, ctx->stream));
        if (dMOD) HIPCHK(hipMemcpyAsync(dMOD, q.dmod, n_dmod * D, hipMemcpyDeviceToHost, ctx->stream));
        return check_unsorted(ctx);             // synchronises
    };
    if ((rc = on_device())) {
        (void)hipStreamSynchronize(ctx->stream);   // whatever was queued from m.hd / m.hi has run before they go
        return rc;
    }
    ctx->dspec_dims[0] = W; ctx->dspec_dims[1] = NPAR; ctx->dspec_dims[2] = L; ctx->dspec_dims[3] = Q;
    ctx->limb_recorded = 1;
    return ANSFM_OK;
}

int ansfm_limb_last(const ansfm_ctx *cctx, double info[3])
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);
    CHECK_CTX(ctx);
    if (!info) FAIL(ANSFM_ERR_INVALID, "limb_last: null argument");
    if (!ctx->limb_recorded) FAIL(ANSFM_ERR_INVALID, "limb_last: no ansfm_cirsradg_ck_limb call recorded yet");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(ctx->limb_ev[2]));
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, ctx->limb_ev[0], ctx->limb_ev[1]));
    HIPCHK(hipEventElapsedTime(&b, ctx->limb_ev[1], ctx->limb_ev[2]));
    info[0] = (double)ctx->limb_scratch_bytes;
    info[1] = a;
    info[2] = b;
    return ANSFM_OK;
}

}  // extern "C"
