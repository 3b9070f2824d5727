// ansfm_limb.hip -- translation unit of the limb-emission kernels (ansfm_limb_kernels.hip.h): the entry point
// ansfm_cirsradg_ck_limb with the build of its index arrays and its launcher, and ansfm_limb_last.  The gas stage it shares with
// the gradient RT entries, the transit entry and the occultation entry is in ansfm_api.hip.  gfx950 only.
#include "ansfm_limb_kernels.hip.h"
#include "ansfm_pathmix.hip.h"

using namespace ansfm;

// k_limb_planck and k_limb_sens, then k_limb_grad, on ctx->stream, between the events limb_last reads
static int launch_limb(ansfm_ctx *ctx, const LimbParams &q, size_t lds_grad)
{
    FusedRoute &r = ctx->limb;
    int rc;
    const unsigned tiles = (unsigned)(q.Wpad / kWave);
    const size_t lds_sens = (size_t)2 * q.L * kWave * sizeof(double);
    if ((rc = ensure_events(ctx, r)) || (rc = allow_lds(ctx, k_limb_sens, lds_sens)) || (rc = allow_lds(ctx, k_limb_grad, lds_grad)))
        return rc;
    HIPCHK(hipEventRecord(r.ev[0], ctx->stream));
    if (q.NT) {
        hipLaunchKernelGGL(k_limb_planck, dim3(tiles, (unsigned)q.NT), dim3(kWave), 0, ctx->stream, q);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_limb_sens, dim3(tiles, (unsigned)(q.Q + (q.n_orphan ? 1 : 0)), (unsigned)q.GS), dim3(kWave), lds_sens, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(r.ev[1], ctx->stream));
    hipLaunchKernelGGL(k_limb_grad, dim3(tiles, (unsigned)q.L), dim3(kMixWaves * kWave), lds_grad, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(r.ev[2], ctx->stream));
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
    const size_t LP = (size_t)LIMAX * P;
    size_t mnz = 0;
    int rc;
    if ((rc = check_mix(ctx, "cirsradg_ck_limb", P, Q, mix_ptr, mix_path, mix_val, &mnz)) ||
        (rc = check_paths(ctx, "cirsradg_ck_limb", L, P, LIMAX, NLAYIN, LAYINC)))
        return rc;
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
    const char *what = "cirsradg_ck_limb";
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, NP1 = ctx->S + 1;
    const size_t D = sizeof(double);
    LimbParams q;
    size_t lds_grad = 0;
    if ((rc = fused_prologue(ctx, what, ctx->limb, L, igas_map, NVMR, NPAR, q, "k_limb_grad", &q.SC, &lds_grad))) return rc;
    // dMOD as a whole, 8 W NPAR L Q bytes, and the scratch beyond the gas stage: B and dB/dT [NT][Wpad] each, spec [P][G][Wpad],
    // dg E [Q][L][G][Wpad], the partial sums of Z [GS][Q][L][Wpad], MOD [W][Q], SPEC [W][P].  A reservation that fails is the
    // caller's cue to take the un-collapsed route.
    const int GS = std::min(G, kLimbGroups);
    const size_t n_tab = m.NT * (size_t)Wpad, n_spec = (size_t)P * G * Wpad, n_out = (size_t)W * ((size_t)Q + P);
    size_t n_dmod = 0, n_E = 0;
    const bool n_E_overflows = __builtin_mul_overflow((size_t)Q * L, (size_t)G * Wpad, &n_E) || n_E > SIZE_MAX / (4 * D);
    if ((rc = reserve_dmod(ctx, what, NPAR, L, Q, n_E_overflows, &n_dmod))) return rc;
    const size_t n_Z = (size_t)GS * Q * L * Wpad;
    const size_t scratch = (2 * n_tab + n_spec + n_E + n_Z + n_out) * D;
    if (ctx->limb.ws.reserve(scratch) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_limb: the scratch (8 Q L G Wpad bytes and smaller arrays) could not be reserved on the device");
    }
    ctx->limb.scratch_bytes = scratch;
    return fused_staged_call(
        ctx, ctx->limb, L, lay_press_pa, lay_temp, amount, taucont, dtaucon, NPAR, Q, m.hd, m.hi, xfac,
        [&](const FusedStaged &s, std::vector<FusedCopy> &copies) -> int {
            const size_t LP = (size_t)LIMAX * P;
            q.tau = ctx->tau.as<double>();
            q.cont = s.cont_t;
            q.delg = ctx->d_delg.as<double>();
            q.xfac = s.xfac;
            q.wave = ctx->d_wave.as<double>();
            q.nlayin = s.di; q.layinc = q.nlayin + P; q.tidx = q.layinc + LP; q.mix_ptr = q.tidx + LP; q.mix_path = q.mix_ptr + Q + 1;
            q.mix_first = q.mix_path + m.mnz; q.orphan = q.mix_first + m.mnz; q.hit = q.orphan + m.n_orphan;
            q.scale = s.dd; q.tvals = s.dd + LP; q.mix_val = q.tvals + m.NT;
            q.btab = ctx->limb.ws.as<double>();
            q.dbtab = q.btab + n_tab;
            q.spec = q.dbtab + n_tab;
            q.E = q.spec + n_spec;
            q.Zp = q.E + n_E;
            q.mod = q.Zp + n_Z;
            q.specout = q.mod + (size_t)W * Q;
            q.dmod = ctx->dspec_ref.as<double>();
            q.dk = ctx->dkbuf.as<double>();
            q.dcont = s.dcont_t;
            q.dcont_gas = s.dcont_gas;
            q.W = W; q.Wpad = Wpad; q.G = G; q.L = L; q.P = P; q.Q = Q;
            q.GS = GS; q.NT = (int)m.NT; q.n_orphan = (int)m.n_orphan; q.ispace = ISPACE;
            q.NPAR = NPAR; q.NVMR = NVMR; q.NP1 = NP1;
            copies = {{MOD, q.mod, (size_t)W * Q * D}, {SPEC, q.specout, (size_t)W * P * D}, {dMOD, q.dmod, n_dmod * D}};
            return ANSFM_OK;
        },
        [&]() { return launch_limb(ctx, q, lds_grad); });
}

int ansfm_limb_last(const ansfm_ctx *ctx, double info[3]) { return fused_last(ctx, &ansfm_ctx::limb, info, "limb"); }

}  // extern "C"
