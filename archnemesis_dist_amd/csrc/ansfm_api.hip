// ansfm_api.hip -- C-ABI of libansfm.so (include/ansfm.h): lifecycle of the context, tables, the gas-opacity stage and the
// thermal / transmission / single-scattering radiative transfer with its gradients.  The other entry points are in
// ansfm_scatter.hip, ansfm_lbl.hip, ansfm_ops.hip, ansfm_mie.hip and ansfm_surface.hip; ansfm_ctx.hip.h is what they share.
// The merge and RT kernels behind these entry points are launched from ansfm_overlap.hip, ansfm_overlapg.hip and ansfm_rt.hip;
// the transit entry point, which shares the gas stage of the gradient entries, is in ansfm_transit.hip.
// gfx950 only.  No CPU fallback: every entry point needs a live HIP device.
#include "ansfm_table_kernels.hip.h"
#include "ansfm_rt_params.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

extern "C" {

int ansfm_abi_version(void) { return ANSFM_ABI_VERSION; }

int ansfm_create(int device, ansfm_ctx **out)
{
    if (!out) return ANSFM_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return ANSFM_ERR_HIP;  // no GPU: there is deliberately no CPU fallback
    ansfm_ctx *ctx = new ansfm_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return ANSFM_ERR_HIP; }
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return ANSFM_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
    for (auto &e : ctx->ev)
        if (hipEventCreate(&e) != hipSuccess) { delete ctx; return ANSFM_ERR_HIP; }
    *out = ctx;
    return ANSFM_OK;
}

void ansfm_destroy(ansfm_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (hipStream_t s : {ctx->stream, ctx->own_stream, ctx->ms_stream, ctx->ms_stream2, ctx->ms_stream3})
        if (s) (void)hipStreamSynchronize(s);
    delete ctx;
}

const char *ansfm_last_error(const ansfm_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int ansfm_set_stream(ansfm_ctx *ctx, void *hip_stream)
{
    CHECK_CTX(ctx);
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return ANSFM_OK;
}

int ansfm_set_gradient_gases(ansfm_ctx *ctx, unsigned int mask)
{
    CHECK_CTX(ctx);
    ctx->grad_gas_mask = mask;
    return ANSFM_OK;
}

int ansfm_set_f32_semantics(ansfm_ctx *ctx, int grid_f32, int delg_f32)
{
    CHECK_CTX(ctx);
    ctx->grid_f32 = grid_f32 ? 1 : 0;
    ctx->delg_f32 = delg_f32 ? 1 : 0;
    return ANSFM_OK;
}

int ansfm_synchronize(ansfm_ctx *ctx)
{
    CHECK_CTX(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* k-table                                                                                     */
/* ------------------------------------------------------------------------------------------ */
// The g-fastest copy of the k-table just written to ctx->lnK (k_table_gfast; OverlapParams::lnKg): built at the end of every
// upload of a k-table, not for one ordinate (G = 1: LBL tables and the line source's stand-in) and not with
// ANSFM_TABLE_GFAST=0 (DESIGN.md 4.1 has the measurement behind the default).  It doubles the table's memory, so an
// allocation that fails is no error: the context is left without the copy and the merge reads lnK as before.  An upload that
// does not build it drops the copy of the table it replaces.
static constexpr bool kTableGfastDefault = true;
static int build_table_gfast(ansfm_ctx *ctx, int Wpad, int G, int Q, bool lbl)
{
    bool want = kTableGfastDefault;
    if (const char *ev = getenv("ANSFM_TABLE_GFAST")) want = ev[0] == '1' ? true : (ev[0] == '0' ? false : want);
    ctx->lnKg_bytes = 0;
    if (!want || lbl || G < 2 || Wpad / kWave > 65535) { ctx->lnKg.release(); return ANSFM_OK; }
    const size_t bytes = (size_t)Q * Wpad * gfast_stride(G) * sizeof(double);
    if (ctx->lnKg.reserve(bytes) != hipSuccess) {
        (void)hipGetLastError();        // clear it: the next HIPCHK(hipGetLastError()) is not about this
        ctx->lnKg.release();
        return ANSFM_OK;
    }
    hipLaunchKernelGGL(k_table_gfast, dim3((unsigned)Q, (unsigned)(Wpad / kWave)), dim3(256), 0, ctx->stream,
                       ctx->lnK.as<double>(), ctx->lnKg.as<double>(), Wpad, G);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->lnKg_bytes = bytes;
    return ANSFM_OK;
}

int ansfm_upload_ktable_dev(ansfm_ctx *ctx, int W, int G, int NP, int NT, int S, const double *K_dev,
                            const double *PRESS, const double *TEMP, const double *WAVE,
                            const double *DELG)
{
    CHECK_CTX(ctx);
    if (W <= 0 || G <= 0 || G > ANSFM_MAX_NG || NP < 2 || NT < 2 || S <= 0 || !K_dev || !PRESS || !TEMP ||
        !WAVE || !DELG)
        FAIL(ANSFM_ERR_INVALID, "upload_ktable: bad dims (need 1<=G<=32, NP>=2, NT>=2) or null pointer");
    HIPCHK(hipSetDevice(ctx->device));
    const int Wpad = round_up(W, kWave);
    const size_t total = (size_t)NP * NT * S * G * Wpad;
    ctx->lnKg_bytes = 0;                 // the copy, if any, is of the table that lnK held
    HIPCHK(ctx->lnK.reserve(total * sizeof(double)));
    HIPCHK(ctx->d_press.reserve(NP * sizeof(double)));
    HIPCHK(ctx->d_temp.reserve(NT * sizeof(double)));
    HIPCHK(ctx->d_wave.reserve((size_t)W * sizeof(double)));
    HIPCHK(ctx->d_delg.reserve(kMaxG * sizeof(double)));
    HIPCHK(ctx->d_flag.reserve(kFlagInts * sizeof(int)));
    HIPCHK(hipMemcpyAsync(ctx->d_press.p, PRESS, NP * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_temp.p, TEMP, NT * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_wave.p, WAVE, (size_t)W * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_delg.p, DELG, G * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_flag.p, 0, kFlagInts * sizeof(int), ctx->stream));
    {
        const int Q = NP * NT * S;
        hipLaunchKernelGGL(k_table_check, dim3(nblk((size_t)W * Q, 256)), dim3(256), 0, ctx->stream, K_dev, W, G, Q,
                           ctx->d_flag.as<int>());
        hipLaunchKernelGGL(k_table_relayout, dim3((unsigned)(Wpad / kWave), nblk((size_t)Q, 64), (unsigned)G), dim3(256), 0,
                           ctx->stream, K_dev, ctx->lnK.as<double>(), W, Wpad, G, Q);
    }
    HIPCHK(hipGetLastError());
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, ctx->d_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->W = W; ctx->Wpad = Wpad; ctx->G = G; ctx->NP = NP; ctx->NT = NT; ctx->S = S;
    ctx->monotone = (flag & 1) ? 0 : 1;
    ctx->has_boxed = (flag & 2) ? 1 : 0;
    ctx->h_delg.assign(DELG, DELG + G);
    ctx->h_wave.assign(WAVE, WAVE + W); ctx->h_press.assign(PRESS, PRESS + NP); ctx->h_temp.assign(TEMP, TEMP + NT);
    ctx->have_table = true;
    ++ctx->table_generation;
    ctx->is_lbl = 0; ctx->temp2d = 0;
    ctx->lblrt = 0; ctx->st_n = 0;       // a table replaces a committed line source
    clear_continuum_sources(ctx);        // they were evaluated on the old table's grid
    return build_table_gfast(ctx, Wpad, G, NP * NT * S, false);
}

int ansfm_upload_ktable(ansfm_ctx *ctx, int W, int G, int NP, int NT, int S, const double *K,
                        const double *PRESS, const double *TEMP, const double *WAVE, const double *DELG)
{
    CHECK_CTX(ctx);
    if (W <= 0 || G <= 0 || NP <= 0 || NT <= 0 || S <= 0 || !K) FAIL(ANSFM_ERR_INVALID, "upload_ktable: bad dims");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)W * G * NP * NT * S;
    HIPCHK(ctx->tmp_in.reserve(n * sizeof(double)));
    HIPCHK(hipMemcpyAsync(ctx->tmp_in.p, K, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    int rc = ansfm_upload_ktable_dev(ctx, W, G, NP, NT, S, ctx->tmp_in.as<double>(), PRESS, TEMP, WAVE, DELG);
    ctx->tmp_in.release();  // the reference-layout copy is only needed during the re-layout
    return rc;
}

/* ---- native .kta reader (Spectroscopy_0.read_ktahead :2492, read_ktable :2733, read_tables :1448) ---------- */
namespace {
struct KtaHeader {
    int irec0 = 0, nwave = 0, npress = 0, ntemp = 0, ng = 0, gasID = 0, isoID = 0;
    double vmin = 0, delv = 0, fwhm = 0;
    std::vector<float> g_ord, del_g, press, temp;
    std::vector<double> wave;
    bool temp2d = false;      // .lta with NT < 0 in the file: one grid of |NT| temperatures per pressure level, temp[npress][ntemp]
};

static double round7(double x) { return std::nearbyint(x * 1e7) / 1e7; }   // np.round(x, decimals=7)

static bool kta_read_header(const char *path, KtaHeader &h, std::string &err)
{
    std::string fn(path);
    if (fn.size() < 4 || fn.compare(fn.size() - 4, 4, ".kta") != 0) fn += ".kta";
    FILE *f = fopen(fn.c_str(), "rb");
    if (!f) { err = "cannot open " + fn; return false; }
    auto rd = [&](void *dst, size_t sz, size_t n) { return fread(dst, sz, n, f) == n; };
    int32_t i4[2]; float f3[3]; int32_t j5[5];
    bool ok = rd(i4, 4, 2) && rd(f3, 4, 3) && rd(j5, 4, 5);
    if (ok) {
        h.irec0 = i4[0]; h.nwave = i4[1];
        h.vmin = round7((double)f3[0]); h.delv = round7((double)f3[1]); h.fwhm = (double)f3[2];
        h.npress = j5[0]; h.ntemp = j5[1]; h.ng = j5[2]; h.gasID = j5[3]; h.isoID = j5[4];
        ok = h.nwave > 0 && h.npress > 0 && h.ntemp > 0 && h.ng > 0 && h.ng <= 1024 && h.irec0 > 0;
        if (!ok) err = "not a k-table header (or NT < 0, a per-pressure temperature grid: .lta only): " + fn;
    } else
        err = "truncated header: " + fn;
    if (ok) {
        float pad[2];
        h.g_ord.resize(h.ng); h.del_g.resize(h.ng); h.press.resize(h.npress); h.temp.resize(h.ntemp);
        ok = rd(h.g_ord.data(), 4, h.ng) && rd(h.del_g.data(), 4, h.ng) && rd(pad, 4, 2) && rd(h.press.data(), 4, h.npress) &&
             rd(h.temp.data(), 4, h.ntemp);
        h.wave.resize(h.nwave);
        if (ok && h.delv > 0.0) {                                   // np.linspace(vmin, vmax, nwave)
            const double vmax = h.delv * (h.nwave - 1) + h.vmin;
            const double step = h.nwave > 1 ? (vmax - h.vmin) / (h.nwave - 1) : 0.0;
            for (int i = 0; i < h.nwave; ++i) h.wave[i] = i * step + h.vmin;
            if (h.nwave > 1) h.wave[h.nwave - 1] = vmax;
        } else if (ok) {
            std::vector<float> wv(h.nwave);
            ok = rd(wv.data(), 4, h.nwave);
            for (int i = 0; i < h.nwave; ++i) h.wave[i] = (double)wv[i];
        }
        if (!ok) err = "truncated header arrays: " + fn;
    }
    fclose(f);
    return ok;
}

// Spectroscopy_0.read_ltahead (:2451): irec0, nwave, vmin, delv, npress, ntemp, gasID, isoID, P, T -- no g-ordinates
// (NG = 1), the wavenumbers always np.linspace(vmin, vmin + delv (nwave-1), nwave) (:2692-2693).
static bool lta_read_header(const char *path, KtaHeader &h, std::string &err)
{
    std::string fn(path);
    if (fn.size() < 4 || fn.compare(fn.size() - 4, 4, ".lta") != 0) fn += ".lta";
    FILE *f = fopen(fn.c_str(), "rb");
    if (!f) { err = "cannot open " + fn; return false; }
    auto rd = [&](void *dst, size_t sz, size_t n) { return fread(dst, sz, n, f) == n; };
    int32_t i2[2]; float f2[2]; int32_t j4[4];
    bool ok = rd(i2, 4, 2) && rd(f2, 4, 2) && rd(j4, 4, 4);
    if (ok) {
        h.irec0 = i2[0]; h.nwave = i2[1];
        h.vmin = round7((double)f2[0]); h.delv = round7((double)f2[1]); h.fwhm = 0.0;
        h.npress = j4[0]; h.ntemp = j4[1]; h.ng = 1; h.gasID = j4[2]; h.isoID = j4[3];
        // NT < 0: the pressure levels are followed by one grid of -NT temperatures per level (:2480-2483, :2684-2687)
        h.temp2d = h.ntemp < 0;
        if (h.temp2d) h.ntemp = -h.ntemp;
        ok = h.nwave > 0 && h.npress > 0 && h.ntemp > 0 && h.irec0 > 0;
        if (!ok) err = "not an LBL-table header: " + fn;
    } else
        err = "truncated header: " + fn;
    if (ok) {
        const size_t ntv = h.temp2d ? (size_t)h.npress * h.ntemp : (size_t)h.ntemp;
        h.g_ord.assign(1, 0.0f); h.del_g.assign(1, 1.0f); h.press.resize(h.npress); h.temp.resize(ntv);
        ok = rd(h.press.data(), 4, h.npress) && rd(h.temp.data(), 4, ntv);
        h.wave.resize(h.nwave);
        const double vmax = h.vmin + h.delv * (h.nwave - 1);
        const double step = h.nwave > 1 ? (vmax - h.vmin) / (h.nwave - 1) : 0.0;
        for (int i = 0; i < h.nwave; ++i) h.wave[i] = i * step + h.vmin;
        if (h.nwave > 1) h.wave[h.nwave - 1] = vmax;
        if (!ok) err = "truncated header arrays: " + fn;
    }
    fclose(f);
    return ok;
}
}  // namespace

int ansfm_lbltable_file_header(const char *path, int64_t dims[3], int32_t ids[2], double hdr[2], double *wave, float *press,
                               float *temp)
{
    if (!path) return ANSFM_ERR_INVALID;
    KtaHeader h; std::string err;
    if (!lta_read_header(path, h, err)) return ANSFM_ERR_INVALID;
    if (dims) { dims[0] = h.nwave; dims[1] = h.npress; dims[2] = h.temp2d ? -h.ntemp : h.ntemp; }    // NT as the file has it
    if (ids) { ids[0] = h.gasID; ids[1] = h.isoID; }
    if (hdr) { hdr[0] = h.vmin; hdr[1] = h.delv; }
    if (wave) memcpy(wave, h.wave.data(), h.wave.size() * sizeof(double));
    if (press) memcpy(press, h.press.data(), h.npress * sizeof(float));
    if (temp) memcpy(temp, h.temp.data(), h.temp.size() * sizeof(float));        // [npress][|NT|] when NT < 0
    return ANSFM_OK;
}

int ansfm_ktable_file_header(const char *path, int64_t dims[4], int32_t ids[2], double hdr[3], double *wave, float *g_ord,
                             float *del_g, float *press, float *temp)
{
    if (!path) return ANSFM_ERR_INVALID;
    KtaHeader h; std::string err;
    if (!kta_read_header(path, h, err)) return ANSFM_ERR_INVALID;
    if (dims) { dims[0] = h.nwave; dims[1] = h.ng; dims[2] = h.npress; dims[3] = h.ntemp; }
    if (ids) { ids[0] = h.gasID; ids[1] = h.isoID; }
    if (hdr) { hdr[0] = h.vmin; hdr[1] = h.delv; hdr[2] = h.fwhm; }
    if (wave) memcpy(wave, h.wave.data(), h.wave.size() * sizeof(double));
    if (g_ord) memcpy(g_ord, h.g_ord.data(), h.ng * sizeof(float));
    if (del_g) memcpy(del_g, h.del_g.data(), h.ng * sizeof(float));
    if (press) memcpy(press, h.press.data(), h.npress * sizeof(float));
    if (temp) memcpy(temp, h.temp.data(), h.ntemp * sizeof(float));
    return ANSFM_OK;
}

static int upload_table_files(ansfm_ctx *ctx, int S, const char *const *paths, double wavemin, double wavemax, bool lta)
{
    CHECK_CTX(ctx);
    if (S <= 0 || !paths) FAIL(ANSFM_ERR_INVALID, "upload_ktable_files: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<KtaHeader> hs(S);
    for (int s = 0; s < S; ++s) {
        std::string err;
        if (!paths[s] || !(lta ? lta_read_header(paths[s], hs[s], err) : kta_read_header(paths[s], hs[s], err)))
            FAIL(ANSFM_ERR_INVALID, "upload_ktable_files: " + err);
        if (hs[s].nwave != hs[0].nwave) FAIL(ANSFM_ERR_INVALID, "error :: Number of wavenumbers in all .kta files must be the same");
        if (hs[s].npress != hs[0].npress) FAIL(ANSFM_ERR_INVALID, "error :: Number of pressure levels in all .kta files must be the same");
        if (hs[s].ntemp != hs[0].ntemp) FAIL(ANSFM_ERR_INVALID, "error :: Number of temperature levels in all .kta files must be the same");
        if (hs[s].ng != hs[0].ng) FAIL(ANSFM_ERR_INVALID, "error :: Number of g-ordinates in all .kta files must be the same");
        if (hs[s].temp2d != hs[0].temp2d) FAIL(ANSFM_ERR_INVALID, "error :: Number of temperature levels in all .kta files must be the same");
    }
    // read_header keeps the grids of the LAST table (:1311-1334); read_tables then cuts WAVE to [wavemin, wavemax]
    // with searchsorted (:1486-1494) and every gas is read over [WAVE.min(), WAVE.max()] of that cut (:1502)
    const KtaHeader &hl = hs[S - 1];
    const int G = hl.ng, NP = hl.npress, NT = hl.ntemp;
    if (G > ANSFM_MAX_NG || NP < 2 || NT < 2) FAIL(ANSFM_ERR_INVALID, "upload_ktable_files: need 1<=G<=32, NP>=2, NT>=2");
    if (lta && NP > 256) FAIL(ANSFM_ERR_UNSUPPORTED, "upload_lbltable_files: NP <= 256");
    const std::vector<double> &wv = hl.wave;
    long iwl = (long)(std::upper_bound(wv.begin(), wv.end(), wavemin) - wv.begin()) - 1;
    if (iwl < 0) iwl = 0;
    long iwh = (long)(std::lower_bound(wv.begin(), wv.end(), wavemax) - wv.begin());
    if (iwh >= (long)wv.size()) iwh = (long)wv.size() - 1;
    if (iwh < iwl) FAIL(ANSFM_ERR_INVALID, "upload_ktable_files: empty wavenumber range");
    const double wlo = wv[iwl], whi = wv[iwh];
    const int W = (int)(iwh - iwl + 1);
    std::vector<double> WAVE(wv.begin() + iwl, wv.begin() + iwh + 1), PRESS(hl.press.begin(), hl.press.end()),
        TEMP(hl.temp.begin(), hl.temp.end()), DELG(hl.del_g.begin(), hl.del_g.end());
    const int Wpad = round_up(W, kWave);
    const size_t total = (size_t)NP * NT * S * G * Wpad;
    ctx->lnKg_bytes = 0;                 // the copy, if any, is of the table that lnK held
    HIPCHK(ctx->lnK.reserve(total * sizeof(double)));
    HIPCHK(ctx->d_press.reserve(NP * sizeof(double)));
    HIPCHK(ctx->d_temp.reserve(TEMP.size() * sizeof(double)));                 // [NP][NT] for a table with NT < 0
    HIPCHK(ctx->d_wave.reserve((size_t)W * sizeof(double)));
    HIPCHK(ctx->d_delg.reserve(kMaxG * sizeof(double)));
    HIPCHK(ctx->d_flag.reserve(kFlagInts * sizeof(int)));
    HIPCHK(hipMemcpyAsync(ctx->d_press.p, PRESS.data(), NP * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_temp.p, TEMP.data(), TEMP.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_wave.p, WAVE.data(), (size_t)W * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_delg.p, DELG.data(), G * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_flag.p, 0, kFlagInts * sizeof(int), ctx->stream));
    const size_t per_wave = (size_t)NP * NT * G;
    std::vector<float> block(per_wave * W);
    HIPCHK(ctx->tmp_in.reserve(block.size() * sizeof(float)));
    for (int s = 0; s < S; ++s) {
        // the wavenumbers of THIS file inside [wlo, whi] (read_ktable :2818-2821) must be the same W points
        const std::vector<double> &ws = hs[s].wave;
        const long a = (long)(std::lower_bound(ws.begin(), ws.end(), wlo) - ws.begin());
        const long b = (long)(std::upper_bound(ws.begin(), ws.end(), whi) - ws.begin());
        if (b - a != W) FAIL(ANSFM_ERR_INVALID, "upload_ktable_files: the tables do not share one wavenumber grid");
        std::string fn(paths[s]);
        const char *ext = lta ? ".lta" : ".kta";
        if (fn.size() < 4 || fn.compare(fn.size() - 4, 4, ext) != 0) fn += ext;
        FILE *f = fopen(fn.c_str(), "rb");
        if (!f) FAIL(ANSFM_ERR_INVALID, "upload_ktable_files: cannot open " + fn);
        const long long off = ((long long)per_wave * a + (hs[s].irec0 - 1)) * 4;     // :2836-2838
        const bool ok = fseeko(f, (off_t)off, SEEK_SET) == 0 && fread(block.data(), 4, block.size(), f) == block.size();
        fclose(f);
        if (!ok) FAIL(ANSFM_ERR_INVALID, "upload_ktable_files: truncated k data in " + fn);
        HIPCHK(hipMemcpyAsync(ctx->tmp_in.p, block.data(), block.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_kta_relayout, dim3(nblk(per_wave * Wpad, 256)), dim3(256), 0, ctx->stream, ctx->tmp_in.as<float>(),
                           ctx->lnK.as<double>(), W, Wpad, G, NP, NT, S, s, ctx->d_flag.as<int>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));                 // `block` is reused for the next gas
    }
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, ctx->d_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->tmp_in.release();
    ctx->W = W; ctx->Wpad = Wpad; ctx->G = G; ctx->NP = NP; ctx->NT = NT; ctx->S = S;
    ctx->monotone = (flag & 1) ? 0 : 1;
    ctx->has_boxed = (flag & 2) ? 1 : 0;
    ctx->h_delg = DELG; ctx->h_wave = WAVE; ctx->h_press = PRESS; ctx->h_temp = TEMP;
    ctx->have_table = true;
    ++ctx->table_generation;
    ctx->is_lbl = lta ? 1 : 0; ctx->temp2d = (lta && hl.temp2d) ? 1 : 0;
    ctx->lblrt = 0; ctx->st_n = 0;
    clear_continuum_sources(ctx);
    if (lta) ctx->monotone = 1;
    ctx->grid_f32 = 1; ctx->delg_f32 = lta ? 0 : 1;   // PRESS / TEMP / DELG come out of the file as float32 arrays (:2544-2559)
    return build_table_gfast(ctx, Wpad, G, NP * NT * S, lta);
}

int ansfm_upload_ktable_files(ansfm_ctx *ctx, int S, const char *const *paths, double wavemin, double wavemax)
{
    return upload_table_files(ctx, S, paths, wavemin, wavemax, false);
}

// Spectroscopy_0.read_lbltable (:2626) for every gas of an ILBL = 2 run: float32 k * 1e20 [wave][press][temp]
int ansfm_upload_lbltable_files(ansfm_ctx *ctx, int S, const char *const *paths, double wavemin, double wavemax)
{
    return upload_table_files(ctx, S, paths, wavemin, wavemax, true);
}

int ansfm_ktable_grids(const ansfm_ctx *ctx, double *WAVE, double *PRESS, double *TEMP, double *DELG)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (!ctx->have_table) return ANSFM_ERR_NOTABLE;
    if (WAVE) memcpy(WAVE, ctx->h_wave.data(), ctx->h_wave.size() * sizeof(double));
    if (PRESS) memcpy(PRESS, ctx->h_press.data(), ctx->h_press.size() * sizeof(double));
    if (TEMP) memcpy(TEMP, ctx->h_temp.data(), ctx->h_temp.size() * sizeof(double));
    if (DELG) memcpy(DELG, ctx->h_delg.data(), ctx->h_delg.size() * sizeof(double));
    return ANSFM_OK;
}

int ansfm_ktable_info(const ansfm_ctx *ctx, int64_t dims[5], int *monotone)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (!ctx->have_table) return ANSFM_ERR_NOTABLE;
    if (dims) { dims[0] = ctx->W; dims[1] = ctx->G; dims[2] = ctx->NP; dims[3] = ctx->NT; dims[4] = ctx->S; }
    if (monotone) *monotone = ctx->monotone;
    return ANSFM_OK;
}

int ansfm_ktable_has_boxed(const ansfm_ctx *ctx, int *has_boxed)
{
    if (!ctx || !has_boxed) return ANSFM_ERR_INVALID;
    if (!ctx->have_table) return ANSFM_ERR_NOTABLE;
    *has_boxed = ctx->has_boxed;
    return ANSFM_OK;
}

int ansfm_last_merge_launch(const ansfm_ctx *ctx, int *waves_per_block, int *trims)
{
    if (!ctx || !waves_per_block || !trims) return ANSFM_ERR_INVALID;
    *waves_per_block = ctx->last_merge.nwaves;
    *trims = ctx->last_merge.trims;
    return ANSFM_OK;
}

int ansfm_last_merge_group_width(const ansfm_ctx *ctx, int *width)
{
    if (!ctx || !width) return ANSFM_ERR_INVALID;
    *width = ctx->last_merge.group_width;
    return ANSFM_OK;
}

int ansfm_last_merge_table_layout(const ansfm_ctx *ctx, int *gfast)
{
    if (!ctx || !gfast) return ANSFM_ERR_INVALID;
    *gfast = ctx->last_merge.gfast ? 1 : 0;
    return ANSFM_OK;
}

int ansfm_ktable_gfast(const ansfm_ctx *ctx, int *present, int64_t *bytes)
{
    if (!ctx || !present || !bytes) return ANSFM_ERR_INVALID;
    if (!ctx->have_table) return ANSFM_ERR_NOTABLE;
    *present = ctx->lnKg_bytes != 0 ? 1 : 0;
    *bytes = (int64_t)ctx->lnKg_bytes;
    return ANSFM_OK;
}

int ansfm_last_merge_rowmajor(const ansfm_ctx *cctx, int64_t *merges, int64_t *merges_total)
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);     // the error text and the stream: nothing of the launch's state changes
    CHECK_CTX(ctx);
    if (!merges || !merges_total) FAIL(ANSFM_ERR_INVALID, "last_merge_rowmajor: null argument");
    *merges = *merges_total = 0;
    if (ctx->d_flag.bytes < kFlagInts * sizeof(int)) return ANSFM_OK;    // nothing has been launched
    HIPCHK(hipSetDevice(ctx->device));
    // the only place the two totals are read: the launch itself gains no stream operation
    unsigned long long v[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(v, ctx->d_flag.as<int>() + kFlagTileCounter + 8, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *merges = (int64_t)v[0];
    *merges_total = (int64_t)v[1];
    return ANSFM_OK;
}

int ansfm_last_merge_order(const ansfm_ctx *cctx, int *applied, int64_t *valid_bytes_nonzero)
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);     // as ansfm_last_merge_rowmajor
    CHECK_CTX(ctx);
    if (!applied || !valid_bytes_nonzero) FAIL(ANSFM_ERR_INVALID, "last_merge_order: null argument");
    *applied = ctx->last_merge_ordered ? 1 : 0;
    *valid_bytes_nonzero = 0;
    if (!ctx->last_merge_ordered || ctx->d_flag.bytes < kFlagInts * sizeof(int)) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long v = 0;                           // the third total behind the tile counters
    HIPCHK(hipMemcpyAsync(&v, ctx->d_flag.as<int>() + kFlagTileCounter + 8 + 4, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *valid_bytes_nonzero = (int64_t)v;
    return ANSFM_OK;
}

int ansfm_last_merge_suffix(const ansfm_ctx *cctx, int64_t *rows, int64_t *rows_of_list_merges)
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);     // as ansfm_last_merge_rowmajor
    CHECK_CTX(ctx);
    if (!rows || !rows_of_list_merges) FAIL(ANSFM_ERR_INVALID, "last_merge_suffix: null argument");
    *rows = *rows_of_list_merges = 0;
    if (ctx->d_flag.bytes < kFlagInts * sizeof(int)) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long v[4] = {0, 0, 0, 0};  // walked merges, all merges, pattern bytes, rows walked behind a list phase
    HIPCHK(hipMemcpyAsync(v, ctx->d_flag.as<int>() + kFlagTileCounter + 8, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *rows = (int64_t)v[3];
    *rows_of_list_merges = (int64_t)(v[1] - v[0]) * ctx->last_merge_G;
    return ANSFM_OK;
}

int ansfm_last_merge_static(const ansfm_ctx *cctx, int64_t *merges, int *valid)
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);     // as ansfm_last_merge_rowmajor
    CHECK_CTX(ctx);
    if (!merges || !valid) FAIL(ANSFM_ERR_INVALID, "last_merge_static: null argument");
    *merges = 0;
    *valid = ctx->last_merge.static_tables ? 1 : 0;
    if (ctx->d_flag.bytes < kFlagInts * sizeof(int)) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long v = 0;                           // the fifth total behind the tile counters
    HIPCHK(hipMemcpyAsync(&v, ctx->d_flag.as<int>() + kFlagTileCounter + 8 + 8, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *merges = (int64_t)v;
    return ANSFM_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* launches                                                                                    */
/* ------------------------------------------------------------------------------------------ */
// src[W][X1][X2] -> dst[(x1, x2) or, swap12, (x2, x1)][Wpad] through a 32 x 32 LDS tile (k_transpose_w_last): both sides move
// whole 256-byte segments.  The element-per-thread version read with a stride of X1 * X2 doubles: 0.18 TB/s, 17.7 of the
// 58 ms of a C3 Jacobian call for the continuum of its 201 states.
static void launch_w_to_last(hipStream_t st, unsigned n_batch, const double *src, double *dst, int W, int Wpad, int X1, int X2,
                             int swap12, double padval, size_t src_stride = 0, size_t dst_stride = 0)
{
    const int X = X1 * X2;
    dim3 grid((unsigned)(Wpad / 32), (unsigned)((X + 31) / 32), n_batch);
    hipLaunchKernelGGL(k_transpose_w_last, grid, dim3(32, 8), 0, st, src, dst, W, Wpad, X1, X2, swap12, padval, src_stride,
                       dst_stride);
}

// Synchronises; *flag = 1 when the fast merge kernel met a k-distribution that is not non-decreasing in g (its
// output is then not to be used: the caller reruns on the generic path, or fails where none exists).
static int read_unsorted(ansfm_ctx *ctx, int *flag)
{
    *flag = 0;
    HIPCHK(hipMemcpyAsync(flag, ctx->d_flag.as<int>() + 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (*flag & 2) FAIL(ANSFM_ERR_HIP, "merge kernel: dynamic LDS does not start at address 0 (unexpected code object layout)");
    *flag &= 1;
    return ANSFM_OK;
}

}  // extern "C": the helpers of the entry points below are templates in places

// Runs run(generic = false) and, if the fast merge met a k-distribution that is not non-decreasing in g, once more with
// run(generic = true): the one rerun policy of the entry points.  The caller cleared the flag before the first pass; the rerun
// clears it again.  Synchronises after each pass.
template <class Run> static int rerun_unsorted(ansfm_ctx *ctx, Run run)
{
    for (int pass = 0; pass < 2; ++pass) {
        if (pass) HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
        int flag = 0, rc = run(pass == 1);
        if (rc || (rc = read_unsorted(ctx, &flag))) return rc;
        if (!flag) break;
    }
    return ANSFM_OK;
}

// The end of an entry point that has no generic path to rerun on: synchronises, ANSFM_ERR_UNSORTED if the fast merge met such a
// k-distribution
int ansfm::check_unsorted(ansfm_ctx *ctx)
{
    int flag = 0, rc = read_unsorted(ctx, &flag);
    if (rc) return rc;
    if (flag)
        FAIL(ANSFM_ERR_UNSORTED, "k-distribution not non-decreasing in g although the table was flagged monotone at upload");
    return ANSFM_OK;
}

// LBL tables: the interpolation records of n_layers layers in ctx->lbl_li
static int lbl_prep(ansfm_ctx *ctx, int n_layers, const double *lay_press, const double *lay_temp, double press_div,
                    int with_grad)
{
    HIPCHK(ctx->lbl_li.reserve((size_t)n_layers * sizeof(LblInterp)));
    hipLaunchKernelGGL(k_layer_prep_lbl, dim3(nblk(n_layers, 128)), dim3(128), 0, ctx->stream, n_layers, lay_press,
                       lay_temp, ctx->NP, ctx->d_press.as<double>(), ctx->NT, ctx->d_temp.as<double>(), ctx->temp2d,
                       press_div, ctx->grid_f32, with_grad, ctx->lbl_li.as<LblInterp>());
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

/* ---- gas opacities of a set of layer rows: calc_k + k_overlap (:3855-3874), or sum_gas k*amount of the LBL tables ------- */
// The rows are device arrays press / temp [n L] and amount [n][S][L], which the merge kernel sees as n models of L layers.
// Two steps, so that the rerun of an unsorted call repeats the merge only.  gas_prep reserves ctx->li / ctx->tau for the rows
// and, for a k-table, interpolates them in its grids (k_layer_prep).
static int gas_prep(ansfm_ctx *ctx, int rows, const double *press, const double *temp)
{
    HIPCHK(ctx->li.reserve((size_t)rows * sizeof(LayerInterp)));
    HIPCHK(ctx->tau.reserve((size_t)rows * ctx->G * ctx->Wpad * sizeof(double)));
    if (ctx->is_lbl) return ANSFM_OK;
    hipLaunchKernelGGL(k_layer_prep, dim3(nblk((size_t)rows, 128)), dim3(128), 0, ctx->stream, rows, press, temp, ctx->NP,
                       ctx->d_press.as<double>(), ctx->NT, ctx->d_temp.as<double>(), 101325.0, ctx->grid_f32,
                       ctx->li.as<LayerInterp>());
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

// gas_tau fills ctx->tau [n L][G][Wpad] by the table's route: k_ck_overlap (generic: every k-distribution sorted first), or
// k_layer_prep_lbl + k_lbl_tau (LBL tables, G = 1, :3795-3817).  dk: the gradient route (k_ck_overlapg / calc_klblg) also
// writes the derivatives [n L][S + 1][G][Wpad] there.
int ansfm::gas_tau(ansfm_ctx *ctx, int n, int L, const double *press, const double *temp, const double *amount, bool generic,
                   double *dk)
{
    ctx->dk_n = dk ? n : 0; ctx->dk_L = L;
    if (ctx->lblrt) {
        // the line source: the rows of ansfm_lblrt_set_state are in ctx->rt_k; press / temp went into them on the host
        const int m0 = ctx->st_m0 >= 0 ? ctx->st_m0 : 0;
        if (ctx->st_n == 0) FAIL(ANSFM_ERR_INVALID, "runtime line-by-line: call ansfm_lblrt_set_state before the CIRSrad call");
        if (L != ctx->st_L || (ctx->st_m0 >= 0 ? m0 + n > ctx->st_n : n != ctx->st_n))
            FAIL(ANSFM_ERR_INVALID, "runtime line-by-line: the call's (n_models, L) = (" + std::to_string(n) + ", " + std::to_string(L) +
                                        ") does not match the state's (" + std::to_string(ctx->st_n) + ", " + std::to_string(ctx->st_L) + ")");
        if (dk && ctx->st_H != 2)
            FAIL(ANSFM_ERR_INVALID, "runtime line-by-line: a gradient call needs the T + 5 K ratios (row_q_*_dT) in ansfm_lblrt_set_state");
        launch_lblrt_tau(ctx, n, L, m0, amount, dk);
        HIPCHK(hipGetLastError());
        return ANSFM_OK;
    }
    if (ctx->is_lbl) {
        const int rows = n * L;
        const int rc = lbl_prep(ctx, rows, press, temp, 101325.0, dk != nullptr);
        if (rc) return rc;
        hipLaunchKernelGGL(k_lbl_tau, dim3(nblk((size_t)rows * ctx->Wpad, 256)), dim3(256), 0, ctx->stream, ctx->lnK.as<double>(),
                           ctx->Wpad, ctx->NT, ctx->S, L, n, ctx->lbl_li.as<LblInterp>(), amount, ctx->tau.as<double>(), dk);
        HIPCHK(hipGetLastError());
        return ANSFM_OK;
    }
    if (dk)
        return launch_overlapg(ctx, false, nullptr, nullptr, ctx->W, ctx->Wpad, ctx->G, ctx->S, L, n, ctx->li.as<LayerInterp>(),
                               amount, ctx->d_delg.as<double>(), ctx->h_delg.data(), ctx->tau.as<double>(), dk, generic);
    return launch_overlap(ctx, false, nullptr, ctx->W, ctx->Wpad, ctx->G, ctx->S, L, n, ctx->li.as<LayerInterp>(), amount,
                          ctx->d_delg.as<double>(), ctx->h_delg.data(), ctx->tau.as<double>(), generic);
}

// The whole stage for `rows` layers of one model, synchronised: a k-table reruns an unsorted call on the generic path; an LBL
// table has no merge and leaves the flag alone
int ansfm::gas_opacity(ansfm_ctx *ctx, int rows, const double *press, const double *temp, const double *amount)
{
    if (!ctx->is_lbl) HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
    int rc = gas_prep(ctx, rows, press, temp);
    if (rc) return rc;
    if (ctx->is_lbl) return gas_tau(ctx, 1, rows, press, temp, amount, false);
    return rerun_unsorted(ctx, [&](bool generic) { return gas_tau(ctx, 1, rows, press, temp, amount, generic); });
}

// Layer de-duplication of a batch of n models x L layers (device rows as above): k_dedup_mark maps every (model, layer) to its
// row in ctx->dd_slot [n][L] -- model 0's L rows first, then the layers in which another model differs (the columns of
// `cols`, what a fused continuum is formed from, take part in the comparison when given) -- the row count is read back
// (synchronises), and k_dedup_gather packs the distinct rows' press, temp [rows] and amount [S][rows] into ctx->dd_in.
int ansfm::dedup_rows(ansfm_ctx *ctx, int n, int L, const double *press, const double *temp, const double *amount,
                      const DedupCols *cols, DedupRows *out)
{
    const int S = ctx->S;
    const size_t nl = (size_t)n * L;
    HIPCHK(ctx->dd_slot.reserve(nl * sizeof(int32_t)));
    HIPCHK(ctx->dd_work.reserve(nl * sizeof(int32_t)));
    int *counter = ctx->d_flag.as<int>() + 12;
    HIPCHK(hipMemsetAsync(counter, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_dedup_mark, dim3(nblk(nl, 128)), dim3(128), 0, ctx->stream, n, L, S, press, temp, amount,
                       ctx->dd_slot.as<int32_t>(), ctx->dd_work.as<int32_t>(), counter, cols ? *cols : DedupCols{});
    HIPCHK(hipGetLastError());
    int extra = 0;
    HIPCHK(hipMemcpyAsync(&extra, counter, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int rows = L + extra;
    HIPCHK(ctx->dd_in.reserve((size_t)rows * (S + 2) * sizeof(double)));
    double *pw = ctx->dd_in.as<double>(), *tw = pw + rows, *aw = tw + rows;
    hipLaunchKernelGGL(k_dedup_gather, dim3(nblk((size_t)rows, 128)), dim3(128), 0, ctx->stream, rows, L, S,
                       ctx->dd_work.as<int32_t>(), press, temp, amount, pw, tw, aw);
    HIPCHK(hipGetLastError());
    *out = DedupRows{rows, pw, tw, aw};
    return ANSFM_OK;
}

// The same with the columns behind the continuum of c (device arrays over the n * L layers).  Without frac_always the para-H2
// fraction counts only where cia_layer reads it (a table with a para-H2 axis): the scattering batch takes a layer from model
// 0's doubling results exactly when its row is model 0's, and a column that changes no opacity must not cost that.
int ansfm::dedup_rows_cont(ansfm_ctx *ctx, int n, int L, const double *press, const double *temp, const double *amount,
                           const ContCall &c, bool frac_always, DedupRows *out)
{
    DedupCols x;
    if (c.ray_mode || c.use_cia) x.add(c.totam, 1);
    if (c.ray_mode == 4) x.add(c.f4, 4);
    if (c.use_cia) {
        x.add(c.q, ctx->cia_NVMR); x.add(c.delh, 1);
        if (frac_always || ctx->cia_NPARA > 0 || ctx->cia_nfrac > 1) x.add(c.frac, 1);
    }
    if (c.use_dust) x.add(c.cont, ctx->dust_n);
    return dedup_rows(ctx, n, L, press, temp, amount, &x, out);
}

// Which slot of the gradient merge (gas i: slot i, temperature: slot S) feeds parameter k of dSPECOUT, for the gradient RT
// kernels and the transit kernels alike; -1: none
int ansfm::fill_slot_of_param(ansfm_ctx *ctx, const int32_t *igas_map_host, int NVMR, int NPAR, unsigned gas_mask,
                              signed char *slot_of_param)
{
    const int S = ctx->S;
    for (int k = 0; k < kMaxPar; ++k) slot_of_param[k] = -1;
    for (int i = 0; i < S; ++i) {   // assignment order of :3868-3870: a later gas overwrites an earlier one
        if (igas_map_host[i] < 0 || igas_map_host[i] >= NPAR) FAIL(ANSFM_ERR_INVALID, "cirsradg: igas_map out of range");
        // a gas that is not selected leaves the parameter to an earlier selected gas of the same column (isotopologues)
        if ((gas_mask >> i) & 1u) slot_of_param[igas_map_host[i]] = (signed char)i;
    }
    slot_of_param[NVMR] = (gas_mask >> 31) ? (signed char)S : (signed char)-1;   // :3872 (written last)
    return ANSFM_OK;
}

// The gas stage of a gradient call on device arrays, for the gradient RT kernels and the transit kernels alike: tau and the
// derivatives of the gradient merge (ctx->tau, ctx->dkbuf; calc_klblg + :3812-3814 for LBL tables) between ev[0] and ev[1], the
// continuum and its gradients transposed to the wave-fastest layouts (cont_t [n][L][Wpad], dcont_t [n][NPAR][L][Wpad], or nullptr)
// -- or, with `fused`, both formed in those layouts from the context's resident sources (k_tau_cont_rows, k_dtau_cont_rows over
// all n * L layers; NVMR: the gas parameters of dTAUCON)
int ansfm::grad_gas_stage(ansfm_ctx *ctx, int n_models, int L, const double *lay_press_pa, const double *lay_temp,
                          const double *amount, const double *taucont, const double *dtaucon, int NPAR, const double **cont_t,
                          const double **dcont_t, const ContCall *fused, int NVMR)
{
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, NP1 = ctx->S + 1;
    *cont_t = *dcont_t = nullptr;
    HIPCHK(ctx->dkbuf.reserve((size_t)n_models * L * NP1 * G * Wpad * sizeof(double)));
    HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
    int rc;
    if ((rc = gas_prep(ctx, n_models * L, lay_press_pa, lay_temp))) return rc;
    if (fused) {
        if ((rc = launch_tau_cont_rows(ctx, n_models * L, nullptr, *fused))) return rc;
        if ((rc = launch_dtau_cont_rows(ctx, n_models, L, NVMR, NPAR, *fused))) return rc;
        *cont_t = ctx->cont_t.as<double>();
        *dcont_t = ctx->dcont_t.as<double>();
    } else if (taucont) {
        HIPCHK(ctx->cont_t.reserve((size_t)n_models * L * Wpad * sizeof(double)));
        launch_w_to_last(ctx->stream, (unsigned)n_models, taucont, ctx->cont_t.as<double>(), W, Wpad, 1, L, 0, 0.0, (size_t)W * L, (size_t)L * Wpad);
        *cont_t = ctx->cont_t.as<double>();
    }
    if (dtaucon) {
        HIPCHK(ctx->dcont_t.reserve((size_t)n_models * NPAR * L * Wpad * sizeof(double)));
        launch_w_to_last(ctx->stream, (unsigned)n_models, dtaucon, ctx->dcont_t.as<double>(), W, Wpad, NPAR, L, 0, 0.0, (size_t)W * NPAR * L, (size_t)NPAR * L * Wpad);
        *dcont_t = ctx->dcont_t.as<double>();
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    if ((rc = gas_tau(ctx, n_models, L, lay_press_pa, lay_temp, amount, false, ctx->dkbuf.as<double>()))) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    return ANSFM_OK;
}

/* ---- the call record of the CIRSrad entry points ---------------------------------------------------------------------- */
namespace {
// What the thermal, transmission, single-scattering and gradient entry points take, under the names and in the layouts of
// include/ansfm.h.  The extern "C" function fills it once and everything below reads it (as MsCall in ansfm_scatter.hip); what
// an entry does not take stays null or 0.  The arrays are host or device pointers as the entry says; igas_map is a host
// pointer always, the arrays of cont the entry's kind as well (stage_call uploads them with the rest).
struct RtCall {
    int ISPACE = 0, n_models = 1, L = 0;
    const double *lay_press_pa = nullptr, *lay_temp = nullptr, *amount = nullptr;
    const double *taucont = nullptr, *tausca = nullptr, *phase = nullptr, *dtaucon = nullptr;
    // the continuum formed inside the call.  fused_cont: (TAUCIA + TAUDUST) + TAURAY (the gradient entries: and dTAUCON; the
    // single-scattering entries: and the scattering opacity and the phase functions) from the context's resident sources, as
    // fused_cont_check left it; without it ray_mode, totam and f4 alone: Rayleigh scattering (ansfm_cirsrad_ck_thermal_ray_dev)
    int fused_cont = 0;
    ContCall cont;
    // ansfm_cirsrad_ck_singlescatt_batch_cont / _src: the populations of phase_fn [W][P][ncont + 1] (host), or alpha_deg [P]
    // (host) to form it from the resident phase-function source
    int ncont = 0;
    const double *phase_fn = nullptr, *alpha_deg = nullptr;
    int NVMR = 0, NPAR = 0;
    const int32_t *igas_map = nullptr;
    int P = 0, LIMAX = 0;
    const int32_t *NLAYIN = nullptr, *LAYINC = nullptr;
    const double *SCALE = nullptr, *EMTEMP = nullptr;
    const double *TSURF = nullptr;          // [n_models]
    const double *EMISSIVITY = nullptr, *SOLFLUX = nullptr, *REFLECTANCE = nullptr, *BRDF = nullptr, *SOL_ANG = nullptr,
                 *EMISS_ANG = nullptr, *xfac = nullptr;
    double *SPECOUT = nullptr, *dSPECOUT = nullptr, *dTSURF = nullptr;
    int rt_mode = 0;                        // RtParams::mode: 0 thermal emission, 1 transmission, 2 single scattering
};

// The host arrays of a call through ctx->hb[], always in this order (an array the entry does not take uploads nothing and
// passes its buffer by): the record returned has the device copies in their place, a null pointer stays null.  igas_map, the
// outputs and the scalars are the caller's.  *rc: the first error.
RtCall stage_call(ansfm_ctx *ctx, const RtCall &h, int *rc)
{
    const size_t W = ctx->W, nl = (size_t)h.n_models * h.L, nlp = (size_t)h.n_models * h.LIMAX * h.P;
    Stager st{ctx};
    RtCall d = h;
    d.lay_press_pa = st.up(h.lay_press_pa, nl); d.lay_temp = st.up(h.lay_temp, nl); d.amount = st.up(h.amount, nl * ctx->S);
    d.taucont = st.up(h.taucont, nl * W); d.tausca = st.up(h.tausca, nl * W); d.phase = st.up(h.phase, nl * W * h.P);
    d.dtaucon = st.up(h.dtaucon, nl * W * h.NPAR);
    d.NLAYIN = st.up(h.NLAYIN, h.P); d.LAYINC = st.up(h.LAYINC, (size_t)h.LIMAX * h.P);
    d.SCALE = st.up(h.SCALE, nlp); d.EMTEMP = st.up(h.EMTEMP, nlp); d.TSURF = st.up(h.TSURF, h.n_models);
    d.EMISSIVITY = st.up(h.EMISSIVITY, W); d.SOLFLUX = st.up(h.SOLFLUX, W); d.REFLECTANCE = st.up(h.REFLECTANCE, W);
    d.BRDF = st.up(h.BRDF, W * h.P); d.SOL_ANG = st.up(h.SOL_ANG, h.P); d.EMISS_ANG = st.up(h.EMISS_ANG, h.P);
    d.xfac = st.up(h.xfac, W);
    d.cont = stage_cont(st, h.cont, nl, d.lay_temp);
    *rc = st.rc;
    return d;
}

// Which (model, layer) opacities a forward call computes: all of them, or (a batch, with de-duplication on) the distinct ones;
// the columns a call forms its continuum from (dedup_rows_cont; frac_always: its rule for the para-H2 fraction) are part of a
// layer's identity.  De-duplicating synchronises.  Records the outcome for ansfm_last_layer_rows / ansfm_get_taugas.
struct GasRows {
    DedupRows k;               // the rows handed to the merge kernel
    int n_k;                   // its view: n_k models of k.rows / n_k layers
    const int32_t *tau_slot;   // [n][L] row of every (model, layer), or nullptr: its own
};
int gas_rows(ansfm_ctx *ctx, const RtCall &c, bool frac_always, GasRows *g)
{
    *g = GasRows{DedupRows{c.n_models * c.L, c.lay_press_pa, c.lay_temp, c.amount}, c.n_models, nullptr};
    if (ctx->dedup && c.n_models > 1 && !ctx->lblrt) {
        const int rc = dedup_rows_cont(ctx, c.n_models, c.L, c.lay_press_pa, c.lay_temp, c.amount, c.cont, frac_always, &g->k);
        if (rc) return rc;
        g->n_k = 1;
        g->tau_slot = ctx->dd_slot.as<int32_t>();
    }
    ctx->last_rows = g->k.rows; ctx->last_dedup = g->tau_slot != nullptr;
    return ANSFM_OK;
}

// The fields of the RT kernels' arguments that come straight from the record (device pointers) and the context, the rest
// zero.  The caller adds what is its own: tau_slot, cont, cont_by_row, sca, phase, mode.
void rt_params_of_call(ansfm_ctx *ctx, const RtCall &c, RtParams &r)
{
    memset(&r, 0, sizeof r);
    r.tau = ctx->tau.as<double>();
    r.wave = ctx->d_wave.as<double>();
    r.delg = ctx->d_delg.as<double>();
    r.nlayin = c.NLAYIN; r.layinc = c.LAYINC; r.scale = c.SCALE; r.emtemp = c.EMTEMP;
    r.lay_press = c.lay_press_pa; r.tsurf = c.TSURF;
    r.emissivity = c.EMISSIVITY; r.solflux = c.SOLFLUX; r.reflectance = c.REFLECTANCE; r.brdf = c.BRDF; r.xfac = c.xfac;
    r.sol_ang = c.SOL_ANG; r.emiss_ang = c.EMISS_ANG;
    r.out = c.SPECOUT;
    r.W = ctx->W; r.Wpad = ctx->Wpad; r.G = ctx->G; r.L = c.L; r.P = c.P; r.LIMAX = c.LIMAX; r.ispace = c.ISPACE;
}

// The one path of the array-level seams (ansfm_thermal_emission, ansfm_singlescatt_plane_spectrum) as two small host vectors
// for them to stage: hi = NLAYIN[1] = Li, LAYINC[Li] = identity; hd = SCALE[Li] = 1, TSURF, SOL_ANG, EMISS_ANG
void identity_path(int Li, double TSURF, double SOL_ANG, double EMISS_ANG, std::vector<int32_t> &hi, std::vector<double> &hd)
{
    hi.assign(1 + Li, Li);
    for (int j = 0; j < Li; ++j) hi[1 + j] = j;
    hd.assign(Li + 3, 1.0);
    hd[Li] = TSURF; hd[Li + 1] = SOL_ANG; hd[Li + 2] = EMISS_ANG;
}
}  // namespace

extern "C" {

/* ------------------------------------------------------------------------------------------ */
/* fused CIRSrad (device pointers)                                                             */
/* ------------------------------------------------------------------------------------------ */
// c.cont.ray_mode: the continuum is Rayleigh scattering alone, of the computed rows (ansfm_cirsrad_ck_thermal_ray_dev); c.fused_cont:
// CIA + aerosols + Rayleigh of the computed rows from the resident sources (ansfm_cirsrad_ck_thermal_cont_dev); c.rt_mode 1:
// the path transmission (ansfm_cirsrad_ck_transmission); generic: the merge sorts every k-distribution first (the rerun of a
// call whose table turned out not to be sorted in g)
static int cirsrad_ck_thermal_dev_impl(ansfm_ctx *ctx, const RtCall &c, bool generic)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsrad: upload a k-table first");
    if (c.n_models <= 0 || c.L <= 0 || c.P <= 0 || c.LIMAX <= 0 || !c.lay_press_pa || !c.lay_temp || !c.amount || !c.NLAYIN ||
        !c.LAYINC || !c.SCALE || !c.EMTEMP || !c.TSURF || !c.SPECOUT || (c.ISPACE != 0 && c.ISPACE != 1))
        FAIL(ANSFM_ERR_INVALID, "cirsrad: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, L = c.L;
    HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
    GasRows g;
    int rc;
    if ((rc = gas_rows(ctx, c, true, &g))) return rc;  // the only synchronisation of this entry point (batches only)
    const int rows = g.k.rows;
    if ((rc = gas_prep(ctx, rows, g.k.press, g.k.temp))) return rc;
    const double *cont_t = nullptr;
    if (c.fused_cont) {
        // CIA, aerosol and Rayleigh opacity of the rows that are computed, from the resident sources
        if ((rc = launch_tau_cont_rows(ctx, rows, g.tau_slot ? ctx->dd_work.as<int32_t>() : (const int32_t *)nullptr, c.cont))) return rc;
        cont_t = ctx->cont_t.as<double>();
    } else if (c.cont.ray_mode) {
        // the Rayleigh continuum of the rows that are computed (the distinct layers of the batch), straight in the layout the RT
        // reads: the 201 states of a C3 Jacobian have 696 of them, not 20 100
        HIPCHK(ctx->cont_t.reserve((size_t)rows * Wpad * sizeof(double)));
        launch_tau_rayleigh_rows(ctx, rows, c.cont.ray_mode, c.ISPACE, g.tau_slot ? ctx->dd_work.as<int32_t>() : (const int32_t *)nullptr,
                                 c.cont.totam, c.cont.f4);
        HIPCHK(hipGetLastError());
        cont_t = ctx->cont_t.as<double>();
    } else if (c.taucont) {
        HIPCHK(ctx->cont_t.reserve((size_t)c.n_models * L * Wpad * sizeof(double)));
        launch_w_to_last(ctx->stream, (unsigned)c.n_models, c.taucont, ctx->cont_t.as<double>(), W, Wpad, 1, L, 0, 0.0, (size_t)W * L, (size_t)L * Wpad);
        HIPCHK(hipGetLastError());
        cont_t = ctx->cont_t.as<double>();
    }
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    if ((rc = gas_tau(ctx, g.n_k, rows / g.n_k, g.k.press, g.k.temp, g.k.amount, generic))) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    RtParams r;
    rt_params_of_call(ctx, c, r);
    r.tau_slot = g.tau_slot;
    r.cont = cont_t;
    r.cont_by_row = ((c.cont.ray_mode || c.fused_cont) && g.tau_slot) ? 1 : 0;
    r.mode = c.rt_mode;
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
    rc = launch_rt(ctx, r, c.n_models);
    if (rc != ANSFM_OK) return rc;
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    call_recorded(ctx, c.n_models, L);
    return ANSFM_OK;
}

int ansfm_cirsrad_ck_thermal_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L,
                                 const double *lay_press_pa, const double *lay_temp,
                                 const double *amount, const double *taucont, int P, int LIMAX,
                                 const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                 const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                 const double *SOLFLUX, const double *REFLECTANCE, const double *SOL_ANG,
                                 const double *EMISS_ANG, const double *xfac, double *SPECOUT)
{
    RtCall c;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.taucont = taucont; c.P = P; c.LIMAX = LIMAX; c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE; c.EMTEMP = EMTEMP;
    c.TSURF = TSURF; c.EMISSIVITY = EMISSIVITY; c.SOLFLUX = SOLFLUX; c.REFLECTANCE = REFLECTANCE; c.SOL_ANG = SOL_ANG;
    c.EMISS_ANG = EMISS_ANG; c.xfac = xfac; c.SPECOUT = SPECOUT;
    return cirsrad_ck_thermal_dev_impl(ctx, c, false);
}

int ansfm_cirsrad_ck_thermal_ray_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                     const double *lay_temp, const double *amount, int ray_mode, const double *TOTAM,
                                     const double *f4, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                     const double *SCALE, const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                     const double *SOLFLUX, const double *REFLECTANCE, const double *SOL_ANG,
                                     const double *EMISS_ANG, const double *xfac, double *SPECOUT)
{
    CHECK_CTX(ctx);
    if ((ray_mode != 1 && ray_mode != 2 && ray_mode != 4 && ray_mode != 12) || !TOTAM || (ray_mode == 4 && !f4))
        FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_thermal_ray_dev: bad argument (ray_mode = IRAY 1, 2, 4 or 12 for calc_tau_rayleighv)");
    RtCall c;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.cont = ContCall{ISPACE, 0, 0, ray_mode, lay_temp, nullptr, nullptr, TOTAM, nullptr, nullptr, ray_mode == 4 ? f4 : nullptr};
    c.P = P; c.LIMAX = LIMAX; c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE; c.EMTEMP = EMTEMP;
    c.TSURF = TSURF; c.EMISSIVITY = EMISSIVITY; c.SOLFLUX = SOLFLUX; c.REFLECTANCE = REFLECTANCE; c.SOL_ANG = SOL_ANG;
    c.EMISS_ANG = EMISS_ANG; c.xfac = xfac; c.SPECOUT = SPECOUT;
    return cirsrad_ck_thermal_dev_impl(ctx, c, false);
}

int ansfm_cirsrad_ck_thermal_cont_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                      const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                      const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                      const double *lay_cont, int ray_mode, const double *f4, int P, int LIMAX,
                                      const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, const double *EMTEMP,
                                      const double *TSURF, const double *EMISSIVITY, const double *SOLFLUX,
                                      const double *REFLECTANCE, const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                                      double *SPECOUT)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsrad: upload a k-table first");
    RtCall c;
    const int rc = fused_cont_check(ctx, "cirsrad_ck_thermal_cont_dev: ", ISPACE, lay_temp, use_cia, lay_q, lay_frac, lay_totam, lay_delh,
                                    use_dust, lay_cont, ray_mode, f4, ContNeed::any_term, &c.cont);
    if (rc) return rc;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.fused_cont = 1;
    c.P = P; c.LIMAX = LIMAX; c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE; c.EMTEMP = EMTEMP;
    c.TSURF = TSURF; c.EMISSIVITY = EMISSIVITY; c.SOLFLUX = SOLFLUX; c.REFLECTANCE = REFLECTANCE; c.SOL_ANG = SOL_ANG;
    c.EMISS_ANG = EMISS_ANG; c.xfac = xfac; c.SPECOUT = SPECOUT;
    return cirsrad_ck_thermal_dev_impl(ctx, c, false);
}

int ansfm_set_layer_dedup(ansfm_ctx *ctx, int enable)
{
    CHECK_CTX(ctx);
    ctx->dedup = enable ? 1 : 0;
    return ANSFM_OK;
}

int ansfm_set_merge_keys(ansfm_ctx *ctx, int bits)
{
    CHECK_CTX(ctx);
    if (bits != 32 && bits != 64) FAIL(ANSFM_ERR_INVALID, "set_merge_keys: bits must be 32 or 64");
    ctx->merge_keys = bits;
    return ANSFM_OK;
}

int ansfm_merge_redo_count(ansfm_ctx *ctx, int64_t *count)
{
    CHECK_CTX(ctx);
    if (!count) FAIL(ANSFM_ERR_INVALID, "merge_redo_count: null argument");
    HIPCHK(hipSetDevice(ctx->device));
    int v = 0;
    HIPCHK(ctx->d_flag.reserve(kFlagInts * sizeof(int)));
    HIPCHK(hipMemcpyAsync(&v, ctx->d_flag.as<int>() + 13, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *count = v;
    return ANSFM_OK;
}

int ansfm_last_layer_rows(const ansfm_ctx *ctx, int *rows_computed, int *rows_total)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (rows_computed) *rows_computed = ctx->last_rows;
    if (rows_total) *rows_total = ctx->last_n * ctx->last_L;
    return ANSFM_OK;
}

int ansfm_last_rt_shared(const ansfm_ctx *ctx, int *shared)
{
    if (!ctx || !shared) return ANSFM_ERR_INVALID;
    *shared = ctx->last_rt_shared;
    return ANSFM_OK;
}

int ansfm_last_kernel_ms(const ansfm_ctx *cctx, double *overlap_ms, int *overlap_launches, double *rt_ms,
                         int *rt_launches)
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);
    CHECK_CTX(ctx);
    if (ctx->overlap_launches == 0) FAIL(ANSFM_ERR_INVALID, "no cirsrad call recorded yet");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(ctx->ev[3]));
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
    HIPCHK(hipEventElapsedTime(&b, ctx->ev[2], ctx->ev[3]));
    ctx->overlap_ms = a; ctx->rt_ms = b;
    if (overlap_ms) *overlap_ms = a;
    if (rt_ms) *rt_ms = b;
    if (overlap_launches) *overlap_launches = ctx->overlap_launches;
    if (rt_launches) *rt_launches = ctx->rt_launches;
    return ANSFM_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* host-pointer wrappers                                                                       */
/* ------------------------------------------------------------------------------------------ */
static int cirsrad_ck_thermal_host(ansfm_ctx *ctx, const RtCall &h)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsrad: upload a k-table first");
    if (h.n_models <= 0 || h.L <= 0 || h.P <= 0 || h.LIMAX <= 0 || !h.SPECOUT) FAIL(ANSFM_ERR_INVALID, "cirsrad: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    int rc;
    RtCall d = stage_call(ctx, h, &rc);
    if (rc) return rc;
    const size_t nout = (size_t)h.n_models * ctx->W * h.P * sizeof(double);
    HIPCHK(ctx->tmp_out.reserve(nout));
    d.SPECOUT = ctx->tmp_out.as<double>();
    rc = rerun_unsorted(ctx, [&](bool generic) { return cirsrad_ck_thermal_dev_impl(ctx, d, generic); });
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h.SPECOUT, ctx->tmp_out.p, nout, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_cirsrad_ck_thermal(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                             const double *lay_temp, const double *amount, const double *taucont, int P,
                             int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                             const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                             const double *SOLFLUX, const double *REFLECTANCE, const double *SOL_ANG,
                             const double *EMISS_ANG, const double *xfac, double *SPECOUT)
{
    RtCall c;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.taucont = taucont; c.P = P; c.LIMAX = LIMAX; c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE; c.EMTEMP = EMTEMP;
    c.TSURF = TSURF; c.EMISSIVITY = EMISSIVITY; c.SOLFLUX = SOLFLUX; c.REFLECTANCE = REFLECTANCE; c.SOL_ANG = SOL_ANG;
    c.EMISS_ANG = EMISS_ANG; c.xfac = xfac; c.SPECOUT = SPECOUT;
    return cirsrad_ck_thermal_host(ctx, c);
}

int ansfm_cirsrad_ck_transmission(ansfm_ctx *ctx, int n_models, int L, const double *lay_press_pa, const double *lay_temp,
                                  const double *amount, const double *taucont, int P, int LIMAX, const int32_t *NLAYIN,
                                  const int32_t *LAYINC, const double *SCALE, const double *xfac, double *SPECOUT)
{
    CHECK_CTX(ctx);
    if (n_models <= 0 || !SCALE) FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_transmission: bad argument");
    std::vector<double> tsurf((size_t)n_models, -1.0);
    RtCall c;
    c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount; c.taucont = taucont;
    c.P = P; c.LIMAX = LIMAX; c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE;
    c.EMTEMP = SCALE;   // the emission temperatures are not used by the transmission epilogue: SCALE stands in for the array
    c.TSURF = tsurf.data(); c.xfac = xfac; c.SPECOUT = SPECOUT; c.rt_mode = 1;
    return cirsrad_ck_thermal_host(ctx, c);
}

int ansfm_get_taugas(ansfm_ctx *ctx, int model, double *TAUGAS)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table || ctx->last_n == 0) FAIL(ANSFM_ERR_INVALID, "get_taugas: no cirsrad call yet");
    if (model < 0 || model >= ctx->last_n || !TAUGAS) FAIL(ANSFM_ERR_INVALID, "get_taugas: bad model index");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, L = ctx->last_L;
    const size_t n = (size_t)W * G * L;
    HIPCHK(ctx->tmp_out.reserve(n * sizeof(double)));
    // internal [L][G][Wpad] -> reference [W][G][L]
    if (ctx->last_dedup)
        hipLaunchKernelGGL(k_taugas_from_slots, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, ctx->tau.as<double>(),
                           ctx->dd_slot.as<int32_t>() + (size_t)model * L, ctx->tmp_out.as<double>(), W, Wpad, L, G);
    else
        hipLaunchKernelGGL(k_w_to_first, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream,
                           ctx->tau.as<double>() + (size_t)model * L * G * Wpad, ctx->tmp_out.as<double>(), W, Wpad, L,
                           G, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(TAUGAS, ctx->tmp_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}


int ansfm_calc_k(ansfm_ctx *ctx, int L, const double *press, const double *temp, double *k_out, double *dkdT_out)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table || ctx->lblrt) FAIL(ANSFM_ERR_NOTABLE, "calc_k: upload a k-table first");
    if (L <= 0 || !press || !temp || !k_out) FAIL(ANSFM_ERR_INVALID, "calc_k: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, S = ctx->S;
    Stager st{ctx};
    const double *dp = st.up(press, L), *dt = st.up(temp, L);
    if (st.rc) return st.rc;
    HIPCHK(ctx->li.reserve((size_t)L * sizeof(LayerInterp)));
    hipLaunchKernelGGL(k_layer_prep, dim3(nblk(L, 128)), dim3(128), 0, ctx->stream, L, dp, dt, ctx->NP, ctx->d_press.as<double>(), ctx->NT, ctx->d_temp.as<double>(),
                       1.0, ctx->grid_f32, ctx->li.as<LayerInterp>());
    const size_t n = (size_t)W * G * L * S;
    HIPCHK(ctx->tmp_out.reserve(n * sizeof(double) * (dkdT_out ? 2 : 1)));
    double *dk = dkdT_out ? ctx->tmp_out.as<double>() + n : nullptr;
    hipLaunchKernelGGL(k_calc_k_seam, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, ctx->lnK.as<double>(), W, Wpad,
                       G, ctx->NT, S, L, ctx->li.as<LayerInterp>(), ctx->tmp_out.as<double>(), dk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(k_out, ctx->tmp_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (dkdT_out) HIPCHK(hipMemcpyAsync(dkdT_out, dk, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_k_overlap(ansfm_ctx *ctx, int W, int G, int L, int S, const double *del_g, const double *k,
                    const double *amount, double *tau)
{
    CHECK_CTX(ctx);
    if (W <= 0 || G <= 0 || G > ANSFM_MAX_NG || L <= 0 || S <= 0 || !del_g || !k || !amount || !tau)
        FAIL(ANSFM_ERR_INVALID, "k_overlap: bad argument (need 1<=G<=32)");
    HIPCHK(hipSetDevice(ctx->device));
    const int Wpad = round_up(W, kWave);
    const size_t nk = (size_t)W * G * L * S;
    Stager st{ctx};
    const double *dk = st.up(k, nk), *dam = st.up(amount, (size_t)S * L), *ddg = st.up(del_g, G);
    if (st.rc) return st.rc;
    HIPCHK(ctx->d_flag.reserve(kFlagInts * sizeof(int)));
    HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
    const size_t nkin = (size_t)S * L * G * Wpad;
    HIPCHK(ctx->tmp_in.reserve(nkin * sizeof(double)));
    hipLaunchKernelGGL(k_kin_permute, dim3(nblk(nkin, 256)), dim3(256), 0, ctx->stream, dk, ctx->tmp_in.as<double>(), W, Wpad, G,
                       L, S);
    HIPCHK(hipGetLastError());
    const size_t ntau = (size_t)L * G * Wpad;
    HIPCHK(ctx->misc.reserve(ntau * sizeof(double)));
    const int rc = rerun_unsorted(ctx, [&](bool generic) {
        return launch_overlap(ctx, true, ctx->tmp_in.as<double>(), W, Wpad, G, S, L, 1, nullptr, dam, ddg, del_g,
                              ctx->misc.as<double>(), generic);
    });
    if (rc) return rc;
    const size_t nout = (size_t)W * G * L;
    HIPCHK(ctx->tmp_out.reserve(nout * sizeof(double)));
    hipLaunchKernelGGL(k_w_to_first, dim3(nblk(nout, 256)), dim3(256), 0, ctx->stream, ctx->misc.as<double>(),
                       ctx->tmp_out.as<double>(), W, Wpad, L, G, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(tau, ctx->tmp_out.p, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_singlescatt_plane_spectrum(ansfm_ctx *ctx, int ISPACE, int W, int G, int NLAYIN, const double *WAVE,
                                     const double *TAUTOT_PATH, const double *TEMP, const double *OMEGA, const double *PHASE,
                                     double TSURF, const double *EMISSIVITY, const double *BRDF, const double *SOLFLUX,
                                     double SOL_ANG, double EMISS_ANG, double *SPECOUT)
{
    CHECK_CTX(ctx);
    if (W <= 0 || G <= 0 || G > ANSFM_MAX_NG || NLAYIN <= 0 || !WAVE || !TAUTOT_PATH || !TEMP || !OMEGA || !PHASE || !SPECOUT ||
        !SOLFLUX || !BRDF || (ISPACE != 0 && ISPACE != 1) || (TSURF > 0.0 && !EMISSIVITY))
        FAIL(ANSFM_ERR_INVALID, "singlescatt_plane_spectrum: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const int Wpad = round_up(W, kWave), Li = NLAYIN;
    const size_t D = sizeof(double);
    std::vector<int32_t> hi;
    std::vector<double> hd;
    identity_path(Li, TSURF, SOL_ANG, EMISS_ANG, hi, hd);
    Stager st{ctx};
    const double *tau = st.up(TAUTOT_PATH, (size_t)W * G * Li), *omega = st.up(OMEGA, (size_t)W * G * Li),
                 *phase = st.up(PHASE, (size_t)W * Li), *temp = st.up(TEMP, Li), *wave = st.up(WAVE, W),
                 *emis = st.up(EMISSIVITY, W), *solflux = st.up(SOLFLUX, W), *brdf = st.up(BRDF, W);
    const int32_t *di = st.up(hi.data(), hi.size());
    const double *dd = st.up(hd.data(), hd.size());
    if (st.rc) return st.rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const size_t ntau = (size_t)Li * G * Wpad;
    HIPCHK(ctx->misc.reserve(2 * ntau * D));
    HIPCHK(ctx->cont_t.reserve((size_t)Li * Wpad * D));
    double *tau_t = ctx->misc.as<double>(), *om_t = tau_t + ntau;
    launch_w_to_last(ctx->stream, (unsigned)1, tau, tau_t, W, Wpad, G, Li, 1, 0.0);
    launch_w_to_last(ctx->stream, (unsigned)1, omega, om_t, W, Wpad, G, Li, 1, 0.0);
    launch_w_to_last(ctx->stream, (unsigned)1, phase, ctx->cont_t.as<double>(), W, Wpad, 1, Li, 0, 0.0);
    HIPCHK(hipGetLastError());
    HIPCHK(ctx->tmp_out.reserve((size_t)W * G * D));
    RtParams r;
    memset(&r, 0, sizeof r);
    r.tau = tau_t; r.omega = om_t; r.phase = ctx->cont_t.as<double>();
    r.wave = wave;
    r.nlayin = di; r.layinc = di + 1;
    r.scale = dd; r.emtemp = temp; r.lay_press = temp;
    r.tsurf = dd + Li;
    r.emissivity = emis; r.solflux = solflux; r.brdf = brdf;
    r.sol_ang = dd + Li + 1; r.emiss_ang = dd + Li + 2;
    r.out = ctx->tmp_out.as<double>();
    r.W = W; r.Wpad = Wpad; r.G = G; r.L = Li; r.P = 1; r.LIMAX = Li; r.ispace = ISPACE; r.per_g = 1; r.mode = 2;
    const int rc = launch_rt(ctx, r, 1);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(SPECOUT, ctx->tmp_out.p, (size_t)W * G * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

// CIRSrad's single-scattering branch for n_models states (host pointers; TSURF [n]): the gas opacities of the distinct (model,
// layer) rows, then mode 2 of k_thermal_rt with the model axis -- the prefix records of state 0 when the batch is de-duplicated
// ss_bad_args: what both implementations refuse alike about the arguments they share.  ss_gas_stage: the gas opacities of the
// rows of the staged call d between ev[0] and ev[1] (frac_always: gas_rows').  ss_rt_stage: mode 2 of k_thermal_rt on the
// continuum, the scattering opacity and the phase functions of s -- by_row: one row of them per gas row, else per (model, layer)
// -- between ev[2] and ev[3], and SPECOUT [n][W][P] to the host; synchronises.
static bool ss_bad_args(const RtCall &h)
{
    bool bad = h.n_models <= 0 || h.L <= 0 || h.P <= 0 || h.LIMAX <= 0 || !h.lay_press_pa || !h.lay_temp || !h.amount || !h.NLAYIN ||
               !h.LAYINC || !h.SCALE || !h.EMTEMP || !h.TSURF || !h.SOLFLUX || !h.SOL_ANG || !h.EMISS_ANG || !h.SPECOUT ||
               (h.ISPACE != 0 && h.ISPACE != 1);
    for (int m = 0; !bad && m < h.n_models; ++m) bad = h.TSURF[m] > 0.0 && !h.EMISSIVITY;
    return bad;
}

static int ss_gas_stage(ansfm_ctx *ctx, const RtCall &d, bool frac_always, GasRows *g)
{
    if (!ctx->is_lbl) HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
    int rc;
    if ((rc = gas_rows(ctx, d, frac_always, g))) return rc;
    const int rows = g->k.rows, n_k = g->n_k;
    ctx->last_n = d.n_models; ctx->last_L = d.L;
    if ((rc = gas_prep(ctx, rows, g->k.press, g->k.temp))) return rc;
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (ctx->is_lbl) rc = gas_tau(ctx, n_k, rows / n_k, g->k.press, g->k.temp, g->k.amount, false);
    else rc = rerun_unsorted(ctx, [&](bool generic) { return gas_tau(ctx, n_k, rows / n_k, g->k.press, g->k.temp, g->k.amount, generic); });
    if (rc) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    return ANSFM_OK;
}

static int ss_rt_stage(ansfm_ctx *ctx, RtCall d, const GasRows &g, const SsContRows &s, bool by_row, double *SPECOUT)
{
    const size_t nout = (size_t)d.n_models * ctx->W * d.P * sizeof(double);
    HIPCHK(ctx->tmp_out.reserve(nout));
    d.SPECOUT = ctx->tmp_out.as<double>();
    RtParams r;
    rt_params_of_call(ctx, d, r);
    r.tau_slot = g.tau_slot; r.cont = s.cont; r.sca = s.sca; r.phase = s.phase;
    if (by_row) { r.cont_by_row = 1; r.ss_by_row = 1; r.rows = g.k.rows; }
    r.mode = d.rt_mode;
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
    const int rc = launch_rt(ctx, r, d.n_models);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    call_recorded(ctx, d.n_models, d.L);
    HIPCHK(hipMemcpyAsync(SPECOUT, ctx->tmp_out.p, nout, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));      // also: the staged host arrays (TSURF of the single entry) are consumed
    return ANSFM_OK;
}

static int cirsrad_ck_singlescatt_impl(ansfm_ctx *ctx, const RtCall &h, const char *fn)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) { ctx->err = std::string(fn) + ": upload a k-table first"; return ANSFM_ERR_NOTABLE; }
    if (ss_bad_args(h) || !h.tausca || !h.phase) { ctx->err = std::string(fn) + ": bad argument"; return ANSFM_ERR_INVALID; }
    if ((size_t)h.n_models * h.P > 65535) { ctx->err = std::string(fn) + ": at most 65535 (model, path) pairs per call"; return ANSFM_ERR_UNSUPPORTED; }
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, n_models = h.n_models, L = h.L, P = h.P;
    const size_t D = sizeof(double), WL = (size_t)W * L, nl = (size_t)n_models * L;
    int rc;
    RtCall d = stage_call(ctx, h, &rc);
    if (rc) return rc;
    GasRows g;
    if ((rc = ss_gas_stage(ctx, d, true, &g))) return rc;
    // reference layouts [n][W][L] -> [n][L][Wpad] (continuum, scattering opacity) and [n][P][W][L] -> [n][P][L][Wpad] (phase)
    const size_t LW = (size_t)L * Wpad;
    HIPCHK(ctx->cont_t.reserve(nl * Wpad * D));
    HIPCHK(ctx->misc.reserve((size_t)n_models * (1 + P) * LW * D));
    double *sca_t = ctx->misc.as<double>(), *ph_t = sca_t + (size_t)n_models * LW;
    const double *cont_t = nullptr;
    if (d.taucont) {
        launch_w_to_last(ctx->stream, (unsigned)n_models, d.taucont, ctx->cont_t.as<double>(), W, Wpad, 1, L, 0, 0.0, WL, LW);
        cont_t = ctx->cont_t.as<double>();
    }
    launch_w_to_last(ctx->stream, (unsigned)n_models, d.tausca, sca_t, W, Wpad, 1, L, 0, 0.0, WL, LW);
    launch_w_to_last(ctx->stream, (unsigned)(n_models * P), d.phase, ph_t, W, Wpad, 1, L, 0, 0.0, WL, LW);
    HIPCHK(hipGetLastError());
    return ss_rt_stage(ctx, d, g, SsContRows{cont_t, sca_t, ph_t}, false, h.SPECOUT);
}

int ansfm_cirsrad_ck_singlescatt(ansfm_ctx *ctx, int ISPACE, int L, const double *lay_press_pa, const double *lay_temp,
                                 const double *amount, const double *taucont, const double *tausca, const double *phase, int P,
                                 int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                 const double *EMTEMP, double TSURF, const double *EMISSIVITY, const double *BRDF,
                                 const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                                 double *SPECOUT)
{
    RtCall c;
    c.ISPACE = ISPACE; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount; c.taucont = taucont;
    c.tausca = tausca; c.phase = phase; c.P = P; c.LIMAX = LIMAX; c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE;
    c.EMTEMP = EMTEMP; c.TSURF = &TSURF; c.EMISSIVITY = EMISSIVITY; c.BRDF = BRDF; c.SOLFLUX = SOLFLUX; c.SOL_ANG = SOL_ANG;
    c.EMISS_ANG = EMISS_ANG; c.xfac = xfac; c.SPECOUT = SPECOUT; c.rt_mode = 2;
    return cirsrad_ck_singlescatt_impl(ctx, c, "cirsrad_ck_singlescatt");
}

int ansfm_cirsrad_ck_singlescatt_batch(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                       const double *lay_temp, const double *amount, const double *taucont, const double *tausca,
                                       const double *phase, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                       const double *SCALE, const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                       const double *BRDF, const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG,
                                       const double *xfac, double *SPECOUT)
{
    RtCall c;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.taucont = taucont; c.tausca = tausca; c.phase = phase; c.P = P; c.LIMAX = LIMAX; c.NLAYIN = NLAYIN; c.LAYINC = LAYINC;
    c.SCALE = SCALE; c.EMTEMP = EMTEMP; c.TSURF = TSURF; c.EMISSIVITY = EMISSIVITY; c.BRDF = BRDF; c.SOLFLUX = SOLFLUX;
    c.SOL_ANG = SOL_ANG; c.EMISS_ANG = EMISS_ANG; c.xfac = xfac; c.SPECOUT = SPECOUT; c.rt_mode = 2;
    return cirsrad_ck_singlescatt_impl(ctx, c, "cirsrad_ck_singlescatt_batch");
}

// The single-scattering batch with the continuum, the scattering opacity and the layer-mean phase functions formed per distinct
// layer from the resident sources (k_ss_cont_rows) and read by row (the SS == 2 builds of k_thermal_rt): the stages of
// cirsrad_ck_singlescatt_impl, one row map for gas opacities and continuum.  h.cont: the nine arguments as the entry took them
// (checked here); h.phase_fn [W][P][ncont + 1] from the host, or h.alpha_deg [P]: formed in its buffer from the resident
// phase-function source (ansfm_cirsrad_ck_singlescatt_batch_src); what = the entry's name
static int cirsrad_ck_singlescatt_cont_impl(ansfm_ctx *ctx, RtCall h, const char *what)
{
    const std::string fn = std::string(what) + ": ";
    const int P = h.P, ncont = h.ncont;
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, fn + "upload a k-table first");
    if (ss_bad_args(h) || (!h.phase_fn && !h.alpha_deg)) FAIL(ANSFM_ERR_INVALID, fn + "bad argument");
    const ContCall a = h.cont;
    int rc = fused_cont_check(ctx, fn, h.ISPACE, h.lay_temp, a.use_cia, a.q, a.frac, a.totam, a.delh, a.use_dust, a.cont, a.ray_mode, a.f4,
                              ContNeed::scatterer, &h.cont);
    if (rc) return rc;
    if (ncont > 7) FAIL(ANSFM_ERR_UNSUPPORTED, fn + "more than 7 aerosol populations (NumPy sums 8 and more pairwise, the kernel sums in order)");
    if (ncont != (a.use_dust ? ctx->dust_n : 0))
        FAIL(ANSFM_ERR_INVALID, fn + "ncont = " + std::to_string(ncont) + " phase functions, the aerosol source has " +
                                    std::to_string(a.use_dust ? ctx->dust_n : 0) + " populations");
    if ((size_t)h.n_models * P > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, fn + "at most 65535 (model, path) pairs per call");
    if (h.alpha_deg && ((rc = phase_source_check(ctx, fn, ncont)) || (rc = phase_source_angles(ctx, fn, P, h.alpha_deg)))) return rc;
    for (int ip = 0; ip < P; ++ip) {                                 // the RT kernel indexes the layers with these
        if (h.NLAYIN[ip] < 1 || h.NLAYIN[ip] > h.LIMAX) FAIL(ANSFM_ERR_INVALID, fn + "NLAYIN outside 1 .. LIMAX");
        for (int j = 0; j < h.NLAYIN[ip]; ++j)
            if (h.LAYINC[(size_t)j * P + ip] < 0 || h.LAYINC[(size_t)j * P + ip] >= h.L) FAIL(ANSFM_ERR_INVALID, fn + "LAYINC entry outside the layer range");
    }
    HIPCHK(hipSetDevice(ctx->device));
    RtCall d = stage_call(ctx, h, &rc);
    if (rc) return rc;
    const size_t npf = (size_t)ctx->W * P * (ncont + 1) * sizeof(double);
    const void *pf_dev = nullptr;
    if (h.alpha_deg) {                                          // phase_fn stays in HBM
        HIPCHK(ctx->ss_phase_fn.reserve(npf));
        if ((rc = launch_phase_source(ctx, P, h.alpha_deg, nullptr, 1, ctx->ss_phase_fn.as<double>()))) return rc;
        pf_dev = ctx->ss_phase_fn.p;
    } else if ((rc = h2d(ctx, ctx->ss_phase_fn, h.phase_fn, npf, &pf_dev)))
        return rc;
    GasRows g;
    if ((rc = ss_gas_stage(ctx, d, false, &g))) return rc;
    SsContRows sr;
    if ((rc = launch_ss_cont_rows(ctx, g.k.rows, g.tau_slot ? ctx->dd_work.as<int32_t>() : (const int32_t *)nullptr, d.cont, P,
                                  static_cast<const double *>(pf_dev), &sr)))
        return rc;
    return ss_rt_stage(ctx, d, g, sr, true, h.SPECOUT);
}

int ansfm_cirsrad_ck_singlescatt_batch_cont(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                            const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                            const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                            const double *lay_cont, int ray_mode, const double *f4, int ncont, const double *phase_fn,
                                            int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                            const double *EMTEMP, const double *TSURF, const double *EMISSIVITY, const double *BRDF,
                                            const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                                            double *SPECOUT)
{
    CHECK_CTX(ctx);
    RtCall c;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.fused_cont = 1; c.cont = ContCall{ISPACE, use_cia, use_dust, ray_mode, lay_temp, lay_q, lay_frac, lay_totam, lay_delh, lay_cont, f4};
    c.ncont = ncont; c.phase_fn = phase_fn;
    c.P = P; c.LIMAX = LIMAX; c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE; c.EMTEMP = EMTEMP; c.TSURF = TSURF;
    c.EMISSIVITY = EMISSIVITY; c.BRDF = BRDF; c.SOLFLUX = SOLFLUX; c.SOL_ANG = SOL_ANG; c.EMISS_ANG = EMISS_ANG; c.xfac = xfac;
    c.SPECOUT = SPECOUT; c.rt_mode = 2;
    return cirsrad_ck_singlescatt_cont_impl(ctx, c, "cirsrad_ck_singlescatt_batch_cont");
}

// The same with phase_fn formed on the device: the populations from the resident phase-function source (ansfm_upload_phase) at
// each path's scattering angle, Rayleigh scattering behind them (k_phase_fn)
int ansfm_cirsrad_ck_singlescatt_batch_src(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                           const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                           const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                           const double *lay_cont, int ray_mode, const double *f4, int ncont, const double *alpha_deg,
                                           int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                           const double *EMTEMP, const double *TSURF, const double *EMISSIVITY, const double *BRDF,
                                           const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                                           double *SPECOUT)
{
    CHECK_CTX(ctx);
    if (!alpha_deg) FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_singlescatt_batch_src: bad argument (alpha_deg)");
    RtCall c;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.fused_cont = 1; c.cont = ContCall{ISPACE, use_cia, use_dust, ray_mode, lay_temp, lay_q, lay_frac, lay_totam, lay_delh, lay_cont, f4};
    c.ncont = ncont; c.alpha_deg = alpha_deg;
    c.P = P; c.LIMAX = LIMAX; c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE; c.EMTEMP = EMTEMP; c.TSURF = TSURF;
    c.EMISSIVITY = EMISSIVITY; c.BRDF = BRDF; c.SOLFLUX = SOLFLUX; c.SOL_ANG = SOL_ANG; c.EMISS_ANG = EMISS_ANG; c.xfac = xfac;
    c.SPECOUT = SPECOUT; c.rt_mode = 2;
    return cirsrad_ck_singlescatt_cont_impl(ctx, c, "cirsrad_ck_singlescatt_batch_src");
}

int ansfm_thermal_emission_g(ansfm_ctx *ctx, int ISPACE, int W, int G, int NPAR, int NLAYIN, const double *WAVE,
                             const double *TAUTOT_PATH, const double *dTAUTOT_PATH, int NVMR, const double *TEMP,
                             const double *PRESS, double TSURF, const double *EMISSIVITY, double *SPECOUT, double *dSPECOUT,
                             double *dTSURF)
{
    CHECK_CTX(ctx);
    if (W <= 0 || G <= 0 || NPAR <= 0 || NLAYIN <= 0 || !WAVE || !TAUTOT_PATH || !dTAUTOT_PATH || !TEMP || !PRESS || !SPECOUT ||
        !dSPECOUT || !dTSURF || (ISPACE != 0 && ISPACE != 1) || (TSURF > 0.0 && !EMISSIVITY))
        FAIL(ANSFM_ERR_INVALID, "thermal_emission_g: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double), WG = (size_t)W * G, Li = NLAYIN;
    Stager st{ctx};
    const double *wave = st.up(WAVE, W), *tau = st.up(TAUTOT_PATH, WG * Li), *dtau = st.up(dTAUTOT_PATH, WG * NPAR * Li),
                 *temp = st.up(TEMP, Li), *press = st.up(PRESS, Li), *emis = st.up(EMISSIVITY, W);
    if (st.rc) return st.rc;
    HIPCHK(ctx->tmp_out.reserve(WG * (2 + (size_t)NPAR * Li) * D));
    double *o_spec = ctx->tmp_out.as<double>(), *o_dts = o_spec + WG, *o_dspec = o_dts + WG;
    launch_thermal_emission_g_seam(ctx, ISPACE, W, G, NPAR, NLAYIN, NVMR, wave, tau, dtau, temp, press, TSURF, emis, o_spec, o_dspec,
                                   o_dts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(SPECOUT, o_spec, WG * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(dTSURF, o_dts, WG * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(dSPECOUT, o_dspec, WG * NPAR * Li * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_thermal_emission(ansfm_ctx *ctx, int ISPACE, int W, int G, int NLAYIN, const double *WAVE,
                           const double *TAUTOT_PATH, const double *EMITOT_PATH, const double *TEMP,
                           const double *PRESS, double TSURF, const double *EMISSIVITY, const double *SOLFLUX,
                           const double *REFLECTANCE, double SOL_ANG, double EMISS_ANG, double *SPECOUT)
{
    CHECK_CTX(ctx);
    if (W <= 0 || G <= 0 || G > ANSFM_MAX_NG || NLAYIN <= 0 || !WAVE || !TAUTOT_PATH || !TEMP || !PRESS || !SPECOUT ||
        (ISPACE != 0 && ISPACE != 1))
        FAIL(ANSFM_ERR_INVALID, "thermal_emission: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const int Wpad = round_up(W, kWave), Li = NLAYIN;
    const size_t D = sizeof(double);
    std::vector<int32_t> hi;
    std::vector<double> hd;
    identity_path(Li, TSURF, SOL_ANG, EMISS_ANG, hi, hd);
    Stager st{ctx};
    const double *tau = st.up(TAUTOT_PATH, (size_t)W * G * Li), *emi = st.up(EMITOT_PATH, (size_t)W * Li),
                 *temp = st.up(TEMP, Li),      // EMTEMP[Li][P=1]
                 *press = st.up(PRESS, Li),    // lay_press[L=Li]
                 *wave = st.up(WAVE, W), *emis = st.up(EMISSIVITY, W), *solflux = st.up(SOLFLUX, W), *refl = st.up(REFLECTANCE, W);
    const int32_t *di = st.up(hi.data(), hi.size());
    const double *dd = st.up(hd.data(), hd.size());
    if (st.rc) return st.rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));  // hi/hd are stack-lifetime host buffers
    // TAUTOT_PATH[W][G][Li] -> tau[Li][G][Wpad]
    const size_t ntau = (size_t)Li * G * Wpad;
    HIPCHK(ctx->misc.reserve(ntau * D));
    launch_w_to_last(ctx->stream, (unsigned)1, tau, ctx->misc.as<double>(), W, Wpad, G, Li, 1, 0.0);
    const double *emi_t = nullptr;
    if (emi) {
        HIPCHK(ctx->cont_t.reserve((size_t)Li * Wpad * D));
        launch_w_to_last(ctx->stream, (unsigned)1, emi, ctx->cont_t.as<double>(), W, Wpad, 1, Li, 0, 0.0);
        emi_t = ctx->cont_t.as<double>();
    }
    HIPCHK(hipGetLastError());
    HIPCHK(ctx->tmp_out.reserve((size_t)W * G * D));
    RtParams r;
    memset(&r, 0, sizeof r);
    r.tau = ctx->misc.as<double>();
    r.emi = emi_t;
    r.wave = wave;
    r.nlayin = di; r.layinc = di + 1;
    r.scale = dd; r.emtemp = temp; r.lay_press = press;
    r.tsurf = dd + Li;
    r.emissivity = emis; r.solflux = solflux; r.reflectance = refl;
    r.sol_ang = dd + Li + 1; r.emiss_ang = dd + Li + 2;
    r.out = ctx->tmp_out.as<double>();
    r.W = W; r.Wpad = Wpad; r.G = G; r.L = Li; r.P = 1; r.LIMAX = Li; r.ispace = ISPACE; r.per_g = 1;
    const int rc = launch_rt(ctx, r, 1);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(SPECOUT, ctx->tmp_out.p, (size_t)W * G * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}


/* ------------------------------------------------------------------------------------------ */
/* gradient path                                                                               */
/* ------------------------------------------------------------------------------------------ */
int ansfm_set_shared_gas_gradient(ansfm_ctx *ctx, int L, const double *dTAU_WL)
{
    CHECK_CTX(ctx);
    ctx->dcont_gas_L = 0;
    if (!dTAU_WL) return ANSFM_OK;
    if (!ctx->have_table || L <= 0) FAIL(ANSFM_ERR_INVALID, "set_shared_gas_gradient: upload a table first; L > 0");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad;
    Stager st{ctx, 12};
    const double *d = st.up(dTAU_WL, (size_t)W * L);
    if (st.rc) return st.rc;
    HIPCHK(ctx->dcont_gas.reserve((size_t)L * Wpad * sizeof(double)));
    launch_w_to_last(ctx->stream, 1u, d, ctx->dcont_gas.as<double>(), W, Wpad, 1, L, 0, 0.0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));      // the staging buffer is reused
    ctx->dcont_gas_L = L;
    return ANSFM_OK;
}

// c.rt_mode 1: the path transmission and its gradients (ansfm_cirsradg_ck_transmission)
static int cirsradg_ck_thermal_dev_impl(ansfm_ctx *ctx, const RtCall &c)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg: upload a k-table first");
    if (c.n_models <= 0 || c.L <= 0 || c.P <= 0 || c.LIMAX <= 0 || !c.lay_press_pa || !c.lay_temp || !c.amount || !c.NLAYIN ||
        !c.LAYINC || !c.SCALE || !c.EMTEMP || !c.TSURF || !c.SPECOUT || !c.dSPECOUT || !c.dTSURF || !c.igas_map || c.NPAR <= 0 ||
        c.NPAR > kMaxPar || c.NVMR < 0 || c.NVMR >= c.NPAR || (c.ISPACE != 0 && c.ISPACE != 1))
        FAIL(ANSFM_ERR_INVALID, "cirsradg: bad argument (NPAR <= 256)");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, n_models = c.n_models, L = c.L, P = c.P, LIMAX = c.LIMAX, NPAR = c.NPAR;
    HIPCHK(ctx->trold_ws.reserve((size_t)n_models * P * (LIMAX + 1) * G * Wpad * sizeof(double)));
    HIPCHK(ctx->dspec_i.reserve((size_t)n_models * P * NPAR * LIMAX * Wpad * sizeof(double)));
    int rc;
    const double *cont_t = nullptr, *dcont_t = nullptr;
    // c.fused_cont: CIA, aerosol and Rayleigh opacity of every layer and their gradients, from the resident sources
    if ((rc = grad_gas_stage(ctx, n_models, L, c.lay_press_pa, c.lay_temp, c.amount, c.taucont, c.dtaucon, NPAR, &cont_t, &dcont_t,
                             c.fused_cont ? &c.cont : nullptr, c.NVMR)))
        return rc;
    RtGParams q;
    memset(&q, 0, sizeof q);
    rt_params_of_call(ctx, c, q.r);
    q.r.cont = cont_t;
    q.r.mode = c.rt_mode;
    q.dk = ctx->dkbuf.as<double>();
    q.dcont = dcont_t;
    if (ctx->dcont_gas_L) {
        if (ctx->dcont_gas_L != L || n_models != 1) {
            ctx->dcont_gas_L = 0;
            FAIL(ANSFM_ERR_INVALID, "cirsradg: the pending shared gas gradient (ansfm_set_shared_gas_gradient) is for one model "
                                    "with a different number of layers");
        }
        q.dcont_gas = ctx->dcont_gas.as<double>();
        ctx->dcont_gas_L = 0;               // one call only
    }
    q.trold_ws = ctx->trold_ws.as<double>();
    q.dspec = ctx->dspec_i.as<double>();
    q.dtsurf = c.dTSURF;
    q.NPAR = NPAR; q.NVMR = c.NVMR; q.NP1 = ctx->S + 1;
    q.gas_mask = ctx->is_lbl ? 0xFFFFFFFFu : ctx->grad_gas_mask;
    if ((rc = fill_slot_of_param(ctx, c.igas_map, c.NVMR, NPAR, q.gas_mask, q.slot_of_param))) return rc;
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
    if ((rc = launch_rtg(ctx, q, n_models))) return rc;
    for (int m = 0; m < n_models; ++m) {
        const size_t nout = (size_t)W * NPAR * LIMAX * P;
        launch_dspec_to_ref(ctx, ctx->dspec_i.as<double>() + (size_t)m * P * NPAR * LIMAX * Wpad, c.dSPECOUT + (size_t)m * nout, W, Wpad,
                            NPAR, LIMAX, P, c.NLAYIN);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    call_recorded(ctx, n_models, L);
    return ANSFM_OK;
}

int ansfm_cirsradg_ck_thermal_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                  const double *lay_temp, const double *amount, const double *taucont,
                                  const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map_host, int P,
                                  int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                  const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                  const double *xfac, double *SPECOUT, double *dSPECOUT, double *dTSURF)
{
    RtCall c;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.taucont = taucont; c.dtaucon = dtaucon; c.NVMR = NVMR; c.NPAR = NPAR; c.igas_map = igas_map_host; c.P = P; c.LIMAX = LIMAX;
    c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE; c.EMTEMP = EMTEMP; c.TSURF = TSURF; c.EMISSIVITY = EMISSIVITY;
    c.xfac = xfac; c.SPECOUT = SPECOUT; c.dSPECOUT = dSPECOUT; c.dTSURF = dTSURF;
    return cirsradg_ck_thermal_dev_impl(ctx, c);
}

// What ansfm_cirsradg_ck_thermal_cont and its _dev twin refuse before anything is staged or launched, and the fields of the
// record that describe the fused continuum
static int grad_fused_cont(ansfm_ctx *ctx, RtCall &c, int use_cia, const double *lay_q, const double *lay_frac, const double *lay_totam,
                           const double *lay_delh, int use_dust, const double *lay_cont, int ray_mode, const double *f4)
{
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg: upload a k-table first");
    if (ctx->dcont_gas_L) {
        // the Rayleigh term is summed into the dense gradients here, (cia + ray) * X: a shared one would be added as a second
        // product
        ctx->dcont_gas_L = 0;
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_thermal_cont: a shared gas gradient (ansfm_set_shared_gas_gradient) is pending; the "
                                "fused continuum forms the Rayleigh term itself (ray_mode).  It has been cancelled.");
    }
    const int rc = fused_cont_check(ctx, "cirsradg_ck_thermal_cont: ", c.ISPACE, c.lay_temp, use_cia, lay_q, lay_frac, lay_totam, lay_delh,
                                    use_dust, lay_cont, ray_mode, f4, ContNeed::any_term, &c.cont);
    if (rc) return rc;
    if (c.NVMR < 0 || c.NPAR < c.NVMR + 2) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_thermal_cont: bad argument (NPAR >= NVMR + 2)");
    if (c.NVMR + 2 > ANSFM_MAX_CONT_GRAD_SLOTS)
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsradg_ck_thermal_cont: NVMR + 2 <= " + std::to_string(ANSFM_MAX_CONT_GRAD_SLOTS) +
                                        " (the gradient slots of a thread are held in LDS)");
    if (use_cia && (c.NVMR != ctx->cia_NVMR || c.NVMR < 2))
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_thermal_cont: NVMR is not the number of gases the CIA source was uploaded for (" +
                                    std::to_string(ctx->cia_NVMR) + "; at least 2: calc_tau_cia writes slot NVMR - 2)");
    if (use_dust && c.NPAR != c.NVMR + 2 + ctx->dust_n)
        FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_thermal_cont: NPAR is not NVMR + 2 + NDUST of the uploaded aerosol source (" +
                                    std::to_string(ctx->dust_n) + " populations)");
    c.fused_cont = 1;
    return ANSFM_OK;
}

static int cirsradg_ck_thermal_host(ansfm_ctx *ctx, const RtCall &h)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg: upload a k-table first");
    if (h.n_models <= 0 || h.L <= 0 || h.P <= 0 || h.LIMAX <= 0 || h.NPAR <= 0 || !h.SPECOUT || !h.dTSURF ||
        (!h.dSPECOUT && h.n_models != 1))
        FAIL(ANSFM_ERR_INVALID, "cirsradg: bad argument (dSPECOUT may be NULL for a single model: the gradients then stay on the "
                                "device for ansfm_map2pro)");
    HIPCHK(hipSetDevice(ctx->device));
    int rc;
    RtCall d = stage_call(ctx, h, &rc);
    if (rc) return rc;
    const size_t D = sizeof(double), nsp = (size_t)h.n_models * ctx->W * h.P, ndsp = nsp * h.NPAR * h.LIMAX;
    HIPCHK(ctx->tmp_out.reserve((2 * nsp) * D));
    HIPCHK(ctx->dspec_ref.reserve(ndsp * D));     // kept on the device for ansfm_map2pro(dSPECIN = NULL)
    ctx->dspec_dims[0] = 0;
    d.SPECOUT = ctx->tmp_out.as<double>(); d.dTSURF = d.SPECOUT + nsp; d.dSPECOUT = ctx->dspec_ref.as<double>();
    if ((rc = cirsradg_ck_thermal_dev_impl(ctx, d))) return rc;
    HIPCHK(hipMemcpyAsync(h.SPECOUT, d.SPECOUT, nsp * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h.dTSURF, d.dTSURF, nsp * D, hipMemcpyDeviceToHost, ctx->stream));
    if (h.dSPECOUT) HIPCHK(hipMemcpyAsync(h.dSPECOUT, ctx->dspec_ref.p, ndsp * D, hipMemcpyDeviceToHost, ctx->stream));
    if (h.n_models == 1) { ctx->dspec_dims[0] = ctx->W; ctx->dspec_dims[1] = h.NPAR; ctx->dspec_dims[2] = h.LIMAX; ctx->dspec_dims[3] = h.P; }
    return check_unsorted(ctx);
}

int ansfm_cirsradg_ck_thermal(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                              const double *lay_temp, const double *amount, const double *taucont,
                              const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P, int LIMAX,
                              const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, const double *EMTEMP,
                              const double *TSURF, const double *EMISSIVITY, const double *xfac, double *SPECOUT,
                              double *dSPECOUT, double *dTSURF)
{
    RtCall c;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.taucont = taucont; c.dtaucon = dtaucon; c.NVMR = NVMR; c.NPAR = NPAR; c.igas_map = igas_map; c.P = P; c.LIMAX = LIMAX;
    c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE; c.EMTEMP = EMTEMP; c.TSURF = TSURF; c.EMISSIVITY = EMISSIVITY;
    c.xfac = xfac; c.SPECOUT = SPECOUT; c.dSPECOUT = dSPECOUT; c.dTSURF = dTSURF;
    return cirsradg_ck_thermal_host(ctx, c);
}

int ansfm_cirsradg_ck_thermal_cont(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                   const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                   const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                   const double *lay_cont, int ray_mode, const double *f4, int NVMR, int NPAR,
                                   const int32_t *igas_map, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                   const double *SCALE, const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                   const double *xfac, double *SPECOUT, double *dSPECOUT, double *dTSURF)
{
    CHECK_CTX(ctx);
    RtCall c;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.NVMR = NVMR; c.NPAR = NPAR; c.igas_map = igas_map; c.P = P; c.LIMAX = LIMAX;
    c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE; c.EMTEMP = EMTEMP; c.TSURF = TSURF; c.EMISSIVITY = EMISSIVITY;
    c.xfac = xfac; c.SPECOUT = SPECOUT; c.dSPECOUT = dSPECOUT; c.dTSURF = dTSURF;
    const int rc = grad_fused_cont(ctx, c, use_cia, lay_q, lay_frac, lay_totam, lay_delh, use_dust, lay_cont, ray_mode, f4);
    return rc ? rc : cirsradg_ck_thermal_host(ctx, c);
}

int ansfm_cirsradg_ck_thermal_cont_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                       const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                       const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                       const double *lay_cont, int ray_mode, const double *f4, int NVMR, int NPAR,
                                       const int32_t *igas_map_host, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                       const double *SCALE, const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                       const double *xfac, double *SPECOUT, double *dSPECOUT, double *dTSURF)
{
    CHECK_CTX(ctx);
    RtCall c;
    c.ISPACE = ISPACE; c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount;
    c.NVMR = NVMR; c.NPAR = NPAR; c.igas_map = igas_map_host; c.P = P; c.LIMAX = LIMAX;
    c.NLAYIN = NLAYIN; c.LAYINC = LAYINC; c.SCALE = SCALE; c.EMTEMP = EMTEMP; c.TSURF = TSURF; c.EMISSIVITY = EMISSIVITY;
    c.xfac = xfac; c.SPECOUT = SPECOUT; c.dSPECOUT = dSPECOUT; c.dTSURF = dTSURF;
    const int rc = grad_fused_cont(ctx, c, use_cia, lay_q, lay_frac, lay_totam, lay_delh, use_dust, lay_cont, ray_mode, f4);
    return rc ? rc : cirsradg_ck_thermal_dev_impl(ctx, c);
}

int ansfm_cirsradg_ck_transmission(ansfm_ctx *ctx, int n_models, int L, const double *lay_press_pa,
                                   const double *lay_temp, const double *amount, const double *taucont,
                                   const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P, int LIMAX,
                                   const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, const double *xfac,
                                   double *SPECOUT, double *dSPECOUT)
{
    CHECK_CTX(ctx);
    if (n_models <= 0 || P <= 0 || !SCALE || !SPECOUT || !dSPECOUT) FAIL(ANSFM_ERR_INVALID, "cirsradg_ck_transmission: bad argument");
    std::vector<double> tsurf((size_t)n_models, -1.0), dts((size_t)n_models * ctx->W * P);
    RtCall c;
    c.n_models = n_models; c.L = L; c.lay_press_pa = lay_press_pa; c.lay_temp = lay_temp; c.amount = amount; c.taucont = taucont;
    c.dtaucon = dtaucon; c.NVMR = NVMR; c.NPAR = NPAR; c.igas_map = igas_map; c.P = P; c.LIMAX = LIMAX; c.NLAYIN = NLAYIN;
    c.LAYINC = LAYINC; c.SCALE = SCALE;
    // no emission in this branch: SCALE stands in for the (unused) emission temperatures, dTSURF is identically zero
    c.EMTEMP = SCALE; c.TSURF = tsurf.data(); c.xfac = xfac; c.SPECOUT = SPECOUT; c.dSPECOUT = dSPECOUT; c.dTSURF = dts.data();
    c.rt_mode = 1;
    return cirsradg_ck_thermal_host(ctx, c);
}

int ansfm_k_overlapg(ansfm_ctx *ctx, int W, int G, int L, int S, const double *del_g, const double *k,
                     const double *dkdT, const double *amount, double *tau, double *dk)
{
    CHECK_CTX(ctx);
    if (W <= 0 || G <= 0 || G > ANSFM_MAX_NG || L <= 0 || S <= 0 || !del_g || !k || !dkdT || !amount || !tau || !dk)
        FAIL(ANSFM_ERR_INVALID, "k_overlapg: bad argument (need 1<=G<=32)");
    HIPCHK(hipSetDevice(ctx->device));
    const int Wpad = round_up(W, kWave), NP1 = S + 1;
    const size_t nk = (size_t)W * G * L * S;
    Stager st{ctx};
    const double *dkk = st.up(k, nk), *dam = st.up(amount, (size_t)S * L), *ddg = st.up(del_g, G), *ddk = st.up(dkdT, nk);
    if (st.rc) return st.rc;
    HIPCHK(ctx->d_flag.reserve(kFlagInts * sizeof(int)));
    HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
    const size_t nkin = (size_t)S * L * G * Wpad;
    HIPCHK(ctx->tmp_in.reserve(nkin * sizeof(double)));
    HIPCHK(ctx->tmp_in2.reserve(nkin * sizeof(double)));
    hipLaunchKernelGGL(k_kin_permute, dim3(nblk(nkin, 256)), dim3(256), 0, ctx->stream, dkk, ctx->tmp_in.as<double>(), W, Wpad, G,
                       L, S);
    hipLaunchKernelGGL(k_kin_permute, dim3(nblk(nkin, 256)), dim3(256), 0, ctx->stream, ddk, ctx->tmp_in2.as<double>(), W, Wpad, G,
                       L, S);
    HIPCHK(hipGetLastError());
    HIPCHK(ctx->misc.reserve((size_t)L * G * Wpad * sizeof(double)));
    HIPCHK(ctx->dkbuf.reserve((size_t)L * NP1 * G * Wpad * sizeof(double)));
    ctx->dk_n = 0;                        // the seam's derivatives replace a CIRSrad call's
    const int rc = rerun_unsorted(ctx, [&](bool generic) {
        return launch_overlapg(ctx, true, ctx->tmp_in.as<double>(), ctx->tmp_in2.as<double>(), W, Wpad, G, S, L, 1, nullptr, dam, ddg,
                               del_g, ctx->misc.as<double>(), ctx->dkbuf.as<double>(), generic);
    });
    if (rc) return rc;
    const size_t nout = (size_t)W * G * L, ndk = nout * NP1;
    HIPCHK(ctx->tmp_out.reserve(nout * sizeof(double)));
    HIPCHK(ctx->tmp_out2.reserve(ndk * sizeof(double)));
    hipLaunchKernelGGL(k_w_to_first, dim3(nblk(nout, 256)), dim3(256), 0, ctx->stream, ctx->misc.as<double>(),
                       ctx->tmp_out.as<double>(), W, Wpad, L, G, 1);
    hipLaunchKernelGGL(k_dk_to_ref, dim3(nblk(ndk, 256)), dim3(256), 0, ctx->stream, ctx->dkbuf.as<double>(),
                       ctx->tmp_out2.as<double>(), W, Wpad, G, L, NP1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(tau, ctx->tmp_out.p, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(dk, ctx->tmp_out2.p, ndk * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return check_unsorted(ctx);
}

/* ------------------------------------------------------------------------------------------ */
/* LBL tables (ILBL = LINE_BY_LINE_TABLES)                                                     */
/* ------------------------------------------------------------------------------------------ */
int ansfm_upload_lbltable(ansfm_ctx *ctx, int W, int NP, int NT, int S, const double *K, const double *PRESS,
                          const double *TEMP, int temp2d, const double *WAVE)
{
    CHECK_CTX(ctx);
    if (W <= 0 || NP < 2 || NT < 2 || S <= 0 || !K || !PRESS || !TEMP || !WAVE)
        FAIL(ANSFM_ERR_INVALID, "upload_lbltable: bad dims (NP>=2, |NT|>=2) or null pointer");
    if (NP > 256) FAIL(ANSFM_ERR_UNSUPPORTED, "upload_lbltable: NP <= 256");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)W * NP * NT * S;
    HIPCHK(ctx->tmp_in.reserve(n * sizeof(double)));
    HIPCHK(hipMemcpyAsync(ctx->tmp_in.p, K, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const double one = 1.0;
    // K[W][NP][NT][S] is the k-table layout with G = 1
    std::vector<double> tfirst(TEMP, TEMP + NT);   // placeholder grid for the generic uploader; replaced below
    int rc = ansfm_upload_ktable_dev(ctx, W, 1, NP, NT, S, ctx->tmp_in.as<double>(), PRESS, tfirst.data(), WAVE, &one);
    ctx->tmp_in.release();
    if (rc) return rc;
    const size_t ntemp = temp2d ? (size_t)NP * NT : (size_t)NT;
    HIPCHK(ctx->d_temp.reserve(ntemp * sizeof(double)));
    HIPCHK(hipMemcpyAsync(ctx->d_temp.p, TEMP, ntemp * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->is_lbl = 1;
    ctx->temp2d = temp2d ? 1 : 0;
    ctx->monotone = 1;
    return ANSFM_OK;
}

int ansfm_calc_klbl(ansfm_ctx *ctx, int L, const double *press, const double *temp, double *k_out, double *dkdT_out)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table || !ctx->is_lbl || ctx->lblrt) FAIL(ANSFM_ERR_NOTABLE, "calc_klbl: upload an LBL table first");
    if (L <= 0 || !press || !temp || !k_out) FAIL(ANSFM_ERR_INVALID, "calc_klbl: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, S = ctx->S;
    Stager st{ctx};
    const double *dp = st.up(press, L), *dt = st.up(temp, L);
    int rc = st.rc;
    if (rc || (rc = lbl_prep(ctx, L, dp, dt, 1.0, dkdT_out != nullptr))) return rc;
    const size_t n = (size_t)W * L * S;
    HIPCHK(ctx->tmp_out.reserve(n * sizeof(double) * (dkdT_out ? 2 : 1)));
    double *dk = dkdT_out ? ctx->tmp_out.as<double>() + n : nullptr;
    hipLaunchKernelGGL(k_calc_klbl_seam, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, ctx->lnK.as<double>(), W, Wpad,
                       ctx->NT, S, L, ctx->lbl_li.as<LblInterp>(), ctx->tmp_out.as<double>(), dk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(k_out, ctx->tmp_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (dkdT_out) HIPCHK(hipMemcpyAsync(dkdT_out, dk, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

}  // extern "C"
