// ansfm_disc.hip -- translation unit of the disc-average kernels (ansfm_disc_kernels.hip.h): the entry point
// ansfm_cirsradg_ck_disc with the build of its index arrays and its launcher, and ansfm_disc_last.  The gas stage it shares with
// the gradient RT entries and the transit, occultation and limb entries is in ansfm_api.hip.  gfx950 only.
#include "ansfm_disc_kernels.hip.h"
#include "ansfm_pathmix.hip.h"

using namespace ansfm;

// k_disc_planck and k_disc_sens, then k_disc_grad, on ctx->stream, between the events disc_last reads
static int launch_disc(ansfm_ctx *ctx, const DiscParams &q, size_t lds_grad)
{
    FusedRoute &r = ctx->disc;
    int rc;
    const unsigned tiles = (unsigned)(q.Wpad / kWave);
    const size_t lds_sens = (size_t)2 * q.L * kWave * sizeof(double);
    if ((rc = ensure_events(ctx, r)) || (rc = allow_lds(ctx, k_disc_sens, lds_sens)) || (rc = allow_lds(ctx, k_disc_grad, lds_grad)))
        return rc;
    HIPCHK(hipEventRecord(r.ev[0], ctx->stream));
    hipLaunchKernelGGL(k_disc_planck, dim3(tiles, (unsigned)q.NT + 1), dim3(kWave), 0, ctx->stream, q);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_disc_sens, dim3(tiles, (unsigned)(q.Q + (q.n_orphan ? 1 : 0)), (unsigned)q.GS), dim3(kWave), lds_sens, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(r.ev[1], ctx->stream));
    hipLaunchKernelGGL(k_disc_grad, dim3(tiles, (unsigned)q.L), dim3(kMixWaves * kWave), lds_grad, ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(r.ev[2], ctx->stream));
    return ANSFM_OK;
}

// What the entry stages of the sequence, the paths and the mix, after checking them.
//   hi = LAYINC [N], tidx [N], mix_ptr [Q + 1], mix_path [mnz], mix_first [mnz], orphan [n_orphan], hit [L Q]
//   hd = SCALE [N P], SCALE by mix entry [N mnz], the distinct EMTEMP values [NT] (distinct as bit patterns, in the order of
//        their first entry), mix_val [mnz], EMISSIVITY [W] where TSURF > 0
struct DiscArrays {
    std::vector<int32_t> hi;
    std::vector<double> hd;
    size_t mnz = 0, n_orphan = 0, NT = 0;
    int ground = 0;
};
static int stage_disc(ansfm_ctx *ctx, int L, const double *lay_press_pa, int N, const int32_t *LAYINC, const double *EMTEMP, int P,
                      const double *SCALE, double TSURF, const double *EMISSIVITY, int Q, const int32_t *mix_ptr, const int32_t *mix_path,
                      const double *mix_val, DiscArrays &m)
{
    size_t mnz = 0;
    int rc;
    if ((rc = check_mix(ctx, "cirsradg_ck_disc", P, Q, mix_ptr, mix_path, mix_val, &mnz))) return rc;
    for (int j = 0; j < N; ++j)
        if (LAYINC[j] < 0 || LAYINC[j] >= L) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_disc: LAYINC outside 0 .. L - 1");
    // the test of :6479-6483 as k_thermal_rtg makes it: a sequence whose last layer lies deeper than its middle one ends at the ground
    int i1 = (int)(N / 2.0) - 1;
    if (i1 < 0) i1 += N;
    m.ground = lay_press_pa[LAYINC[N - 1]] > lay_press_pa[LAYINC[i1]];
    std::vector<char> named(P, 0);
    std::vector<int32_t> first(mnz, 0), orphan;
    for (size_t i = 0; i < mnz; ++i)
        if (!named[mix_path[i]]) { named[mix_path[i]] = 1; first[i] = 1; }
    for (int p = 0; p < P; ++p)
        if (!named[p]) orphan.push_back(p);
    std::map<uint64_t, int32_t> seen;
    std::vector<double> tvals;
    std::vector<int32_t> tidx(N, 0);
    for (int j = 0; j < N; ++j) {
        uint64_t bits;
        memcpy(&bits, &EMTEMP[j], sizeof bits);
        auto it = seen.find(bits);
        if (it == seen.end()) {
            it = seen.emplace(bits, (int32_t)tvals.size()).first;
            tvals.push_back(EMTEMP[j]);
        }
        tidx[j] = it->second;
    }
    if (tvals.size() > 65534) FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_disc: more than 65534 distinct EMTEMP values");
    std::vector<int32_t> hit((size_t)L * Q, 0);
    for (int q = 0; q < Q; ++q)
        if (mix_ptr[q + 1] > mix_ptr[q])
            for (int j = 0; j < N; ++j) hit[(size_t)LAYINC[j] * Q + q] = 1;
    m.mnz = mnz; m.n_orphan = orphan.size(); m.NT = tvals.size();
    m.hi.assign(LAYINC, LAYINC + N);
    m.hi.insert(m.hi.end(), tidx.begin(), tidx.end());
    m.hi.insert(m.hi.end(), mix_ptr, mix_ptr + Q + 1);
    m.hi.insert(m.hi.end(), mix_path, mix_path + mnz);
    m.hi.insert(m.hi.end(), first.begin(), first.end());
    m.hi.insert(m.hi.end(), orphan.begin(), orphan.end());
    m.hi.insert(m.hi.end(), hit.begin(), hit.end());
    m.hd.assign(SCALE, SCALE + (size_t)N * P);
    for (int j = 0; j < N; ++j)
        for (size_t i = 0; i < mnz; ++i) m.hd.push_back(SCALE[(size_t)j * P + mix_path[i]]);
    m.hd.insert(m.hd.end(), tvals.begin(), tvals.end());
    m.hd.insert(m.hd.end(), mix_val, mix_val + mnz);
    if (TSURF > 0.0) m.hd.insert(m.hd.end(), EMISSIVITY, EMISSIVITY + ctx->W);
    return ANSFM_OK;
}

extern "C" {

// Disc-averaged thermal emission with gradients of one model and one geometry set (nemesisdiscfmg, ForwardModel_0.py:1719-1834),
// the averaging points mixed to the Q geometries on the device: the gas stage of the gradient RT entries (grad_gas_stage), then
// k_disc_planck, k_disc_sens and k_disc_grad.  Neither trold_ws nor dspec_i nor the scratch of the other fused entries is
// touched; dMOD (W, NPAR, L, Q) stays in dspec_ref for ansfm_map2pro(dSPECIN = NULL).
int ansfm_cirsradg_ck_disc(ansfm_ctx *ctx, int ISPACE, int L, const double *lay_press_pa, const double *lay_temp, const double *amount,
                           const double *taucont, const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int N,
                           const int32_t *LAYINC, const double *EMTEMP, int P, const double *SCALE, double TSURF,
                           const double *EMISSIVITY, int Q, const int32_t *mix_ptr, const int32_t *mix_path, const double *mix_val,
                           const double *xfac, double *MOD, double *SPEC, double *dTSMOD, double *dMOD)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg_ck_disc: upload a k-table first");
    if (L <= 0 || N <= 0 || P <= 0 || Q <= 0 || !lay_press_pa || !lay_temp || !amount || !LAYINC || !SCALE || !EMTEMP || !mix_ptr ||
        !MOD || !igas_map || NPAR <= 0 || NPAR > kMaxPar || NVMR < 0 || NVMR >= NPAR || (ISPACE != 0 && ISPACE != 1))
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_disc: bad argument (N, P, Q > 0, NPAR <= 256, ISPACE 0 or 1)");
    if (TSURF > 0.0 && !EMISSIVITY) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_disc: TSURF > 0 needs EMISSIVITY");
    if (L > kDiscMaxLayers)
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_disc: at most 160 layers (the two 64-lane LDS rows per layer of k_disc_sens, 160 KiB)");
    if (Q > 65534) FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_disc: more than 65534 geometries");
    DiscArrays m;
    int rc;
    if ((rc = stage_disc(ctx, L, lay_press_pa, N, LAYINC, EMTEMP, P, SCALE, TSURF, EMISSIVITY, Q, mix_ptr, mix_path, mix_val, m))) return rc;

    // everything that can refuse the arguments comes before the first copy is queued
    const char *what = "cirsradg_ck_disc";
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, NP1 = ctx->S + 1;
    const size_t D = sizeof(double);
    DiscParams q;
    size_t lds_grad = 0;
    if ((rc = fused_prologue(ctx, what, ctx->disc, L, igas_map, NVMR, NPAR, q, "k_disc_grad", &q.SC, &lds_grad))) return rc;
    // dMOD as a whole, 8 W NPAR L Q bytes, and the scratch beyond the gas stage: B and dB/dT [NT + 1][Wpad] each, spec [P][G][Wpad],
    // dg E [Q][L][G][Wpad], the partial sums of Z [GS][Q][L][Wpad], the ground's sums [Q][G][Wpad], MOD and dTSMOD [W][Q], SPEC
    // [W][P].  A reservation that fails is the caller's cue to take the un-collapsed route.
    const int GS = disc_groups(G, Wpad / kWave, Q + (m.n_orphan ? 1 : 0));
    const size_t n_tab = (m.NT + 1) * (size_t)Wpad, n_spec = (size_t)P * G * Wpad, n_tsg = (size_t)Q * G * Wpad,
                 n_out = (size_t)W * (2 * (size_t)Q + P);
    size_t n_dmod = 0, n_E = 0;
    const bool n_E_overflows = __builtin_mul_overflow((size_t)Q * L, (size_t)G * Wpad, &n_E) || n_E > SIZE_MAX / (4 * D);
    if ((rc = reserve_dmod(ctx, what, NPAR, L, Q, n_E_overflows, &n_dmod))) return rc;
    const size_t n_Z = (size_t)GS * Q * L * Wpad;
    const size_t scratch = (2 * n_tab + n_spec + n_E + n_Z + n_tsg + n_out) * D;
    if (ctx->disc.ws.reserve(scratch) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_disc: the scratch (8 Q L G Wpad bytes and smaller arrays) could not be reserved on the device");
    }
    ctx->disc.scratch_bytes = scratch;
    rc = fused_staged_call(
        ctx, ctx->disc, L, lay_press_pa, lay_temp, amount, taucont, dtaucon, NPAR, Q, m.hd, m.hi, xfac,
        [&](const FusedStaged &s, std::vector<FusedCopy> &copies) -> int {
            const size_t NP_ = (size_t)N * P;
            q.tau = ctx->tau.as<double>();
            q.cont = s.cont_t;
            q.delg = ctx->d_delg.as<double>();
            q.xfac = s.xfac;
            q.wave = ctx->d_wave.as<double>();
            q.layinc = s.di; q.tidx = q.layinc + N; q.mix_ptr = q.tidx + N; q.mix_path = q.mix_ptr + Q + 1;
            q.mix_first = q.mix_path + m.mnz; q.orphan = q.mix_first + m.mnz; q.hit = q.orphan + m.n_orphan;
            q.scale = s.dd; q.smix = s.dd + NP_; q.tvals = q.smix + (size_t)N * m.mnz; q.mix_val = q.tvals + m.NT;
            q.emis = TSURF > 0.0 ? q.mix_val + m.mnz : nullptr;
            q.btab = ctx->disc.ws.as<double>();
            q.dbtab = q.btab + n_tab;
            q.spec = q.dbtab + n_tab;
            q.E = q.spec + n_spec;
            q.Zp = q.E + n_E;
            q.tsg = q.Zp + n_Z;
            q.mod = q.tsg + n_tsg;
            q.dtsmod = q.mod + (size_t)W * Q;
            q.specout = q.dtsmod + (size_t)W * Q;
            q.dmod = ctx->dspec_ref.as<double>();
            q.dk = ctx->dkbuf.as<double>();
            q.dcont = s.dcont_t;
            q.dcont_gas = s.dcont_gas;
            q.tsurf = TSURF;
            q.W = W; q.Wpad = Wpad; q.G = G; q.L = L; q.P = P; q.Q = Q; q.N = N; q.mnz = (int)m.mnz;
            q.GS = GS; q.NT = (int)m.NT; q.n_orphan = (int)m.n_orphan; q.ispace = ISPACE; q.ground = m.ground;
            q.NPAR = NPAR; q.NVMR = NVMR; q.NP1 = NP1;
            copies = {{MOD, q.mod, (size_t)W * Q * D}, {SPEC, q.specout, (size_t)W * P * D}, {dTSMOD, q.dtsmod, (size_t)W * Q * D},
                      {dMOD, q.dmod, n_dmod * D}};
            return ANSFM_OK;
        },
        [&]() { return launch_disc(ctx, q, lds_grad); });
    if (rc) return rc;
    // the stream is idle here (the staged call synchronised): the times between the events are read once and kept with the
    // record, so that ansfm_disc_last returns the same numbers however often and whenever it is asked
    float a = 0.f, b = 0.f;
    ctx->disc.recorded = 0;
    HIPCHK(hipEventElapsedTime(&a, ctx->disc.ev[0], ctx->disc.ev[1]));
    HIPCHK(hipEventElapsedTime(&b, ctx->disc.ev[1], ctx->disc.ev[2]));
    ctx->disc.ms[0] = a; ctx->disc.ms[1] = b;
    ctx->disc.recorded = 1;
    return ANSFM_OK;
}

int ansfm_disc_last(const ansfm_ctx *cctx, double info[3])
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);
    CHECK_CTX(ctx);
    if (!info) FAIL(ANSFM_ERR_INVALID, "disc_last: null argument");
    if (!ctx->disc.recorded) FAIL(ANSFM_ERR_INVALID, "disc_last: no ansfm_cirsradg_ck_disc call recorded yet");
    info[0] = (double)ctx->disc.scratch_bytes;
    info[1] = ctx->disc.ms[0];
    info[2] = ctx->disc.ms[1];
    return ANSFM_OK;
}

}  // extern "C"
