// ansfm_api.hip -- C-ABI of libansfm.so (include/ansfm.h): context, HBM buffers, launches.
// gfx950 only.  No CPU fallback: every entry point needs a live HIP device.
#include "ansfm_kernels.hip.h"
#include "ansfm_ms_kernels.hip.h"
#include "ansfm_ms_lane.hip.h"
#include "ansfm_lbl_kernels.hip.h"
#include "ansfm_lbl_pc_kernels.hip.h"
#include "ansfm_lblrt_kernels.hip.h"
#include "ansfm_mie_kernels.hip.h"
#include "ansfm_layer_kernels.hip.h"
#include "ansfm_map_kernels.hip.h"
#include "ansfm_conv_kernels.hip.h"
#include "ansfm_cont_kernels.hip.h"
#include "ansfm_kdist.hip.h"
#include "ansfm_merge32_launch.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/ansfm.h"
#pragma GCC visibility pop

using namespace ansfm;

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n)
    {
        if (n <= bytes) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; bytes = 0; }
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// One isotopologue of the runtime line source (ansfm_lblrt_*): everything that stays fixed over a retrieval, in HBM
struct LblrtIso {
    int lineshape_id = 0, include_lines = 0, include_continuum = 0;
    double abundance = 0, mass = 0;
    int N = 0;                           // lines, sorted by wavenumber: lines = nu, sw, e_lower, stim_ref [N], bparams [3M][N]
    double t_ref = 0, p_ref = 0, s_floor = 0, wn_calc_window = 0, wn_approx_window = 0;
    DevBuf lines;
    std::vector<double> dabs;            // [M] the largest |delta| of a broadener over the lines: bounds the pressure shift
    int Nb = 0, nb = 0;                  // pseudo-continuum bins: bins = centers, widths, sw_sum, e_lower, lo [Nb], bparams [3M][Nb]
    int first = 0, last = 0, jmax = 0;
    double t_cont = 0, p_cont = 0, wmax = 0;
    DevBuf bins;
};

}  // namespace

struct ansfm_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    int num_cus = 256;

    // k-table
    int W = 0, Wpad = 0, G = 0, NP = 0, NT = 0, S = 0;
    int monotone = 0;
    int has_boxed = 1;        // some table entry is <= 0 or NaN (stored NaN-boxed, encode_lnk); 0 selects the box-free load path
    std::vector<double> h_wave, h_press, h_temp;   // host copies of the grids of the table in HBM
    DevBuf dcont_gas;                       // ansfm_set_shared_gas_gradient: [L][Wpad], consumed by the next cirsradg call
    int dcont_gas_L = 0;                    // 0: none pending
    unsigned grad_gas_mask = 0xFFFFFFFFu;   // ansfm_set_gradient_gases: gases whose amount gradients cirsradg computes
    int merge_keys = 64;     // 32: run the forward merge on k_ck_overlap32's float32 keys (ansfm_set_merge_keys)
    bool have_table = false;
    int grid_f32 = 0, delg_f32 = 0;
    int is_lbl = 0, temp2d = 0;   // LBL-table mode (ILBL=2): G = 1, TEMP may be [NP][NT]
    DevBuf lnK, d_press, d_temp, d_wave, d_delg, d_flag;
    std::vector<double> h_delg;

    // workspaces
    DevBuf li, tau, scratch, cont_t, tmp_in, tmp_out, misc;
    DevBuf dspec_ref, map_out, map_b, map_batch;
    DevBuf dd_slot, dd_work, dd_in;      // layer de-duplication: row map [n][L], work list, packed inputs
    DevBuf ms_radg16, ms_brdf16;         // 7 .. 15 streams padded to the 16-stream kernels' layout
    DevBuf rt_prefix, rt_same;           // thermal RT of a batch: state 0's records along every path; same flags [n][L] (single scattering: [n][P][L]) + jstart [n][P]
    int last_rt_shared = 0;
    int dedup = 1;                       // ansfm_set_layer_dedup
    int last_rows = 0, last_dedup = 0;   // opacity rows computed by the last cirsrad call / whether tau_slot applies
    int dspec_dims[4] = {0, 0, 0, 0};   // W, NPAR, LIMAX, P of dspec_ref (single-model cirsradg result)
    int map_dims[4] = {0, 0, 0, 0};     // W, NPAR, NPRO, P of map_out
    DevBuf gscratch, perm, dkbuf, trold_ws, dspec_i, dcont_t, tmp_in2, tmp_out2, lbl_li;
    DevBuf ms_taus, ms_omegas, ms_bnu;   // scattering branch of CIRSrad: TAUTOT / OMEGA (W,G,L) and BB (W,L) in HBM
    DevBuf ms_tauray_l, ms_lfrac_l;      // the continuum by rows: TAURAY / aerosol fractions of a launch's models (the model-by-model route: one model's dense arrays)
    DevBuf ms_cache, ms_orders, ms_same, ms_pcache, ms_lstart; // batched scattering Jacobian: doubled layers / prefix stacks of model 0, orders cached, layer flags, sweep starts
    long ms_cache_hits = 0, ms_cache_layers = 0;   // (model, layer) pairs taken from the cache / all, last batch call
    long ms_windows = 0, ms_window_w = 0;          // spectral windows of phase matrices / Hansen factors of the last scattering call, their size
    DevBuf hb[24];  // staging buffers of the host-pointer entry points
    // runtime line-by-line: the opacity of a gas, summed in HBM (ansfm_lbl_accum_*); its grid and (T, p) points [2][L]
    DevBuf acc, acc_grid, acc_tp;
    int acc_nw = 0, acc_L = 0;           // 0: no accumulator begun
    std::vector<double> acc_h_grid, acc_h_p;
    int last_n = 0, last_L = 0;
    int dk_n = 0, dk_L = 0;              // models / layers of the gas-opacity derivatives in dkbuf (ansfm_get_dtaugas); 0: none
    // runtime line-by-line as the context's opacity source (ansfm_lblrt_*): 0 none, 1 begun, 2 committed; lblrt: the
    // committed source stands in for the table (is_lbl = 1, G = 1, W = nw) until a table is uploaded
    int rt_stage = 0, lblrt = 0, rt_nw = 0, rt_S = 0, rt_M = 0;
    std::vector<double> rt_h_grid;
    DevBuf rt_grid, rt_k, rt_pts, rt_scratch, rt_krow;   // grid; k rows [R][H][nw]; staged points; line / bin constants; krow [n][S][L]
    std::vector<std::vector<std::unique_ptr<LblrtIso>>> rt_gas;   // [S][isotopologues]
    size_t rt_budget = (size_t)256 << 20;                // bytes of rt_scratch a chunk of rows may take
    int st_n = 0, st_L = 0, st_R = 0, st_H = 0;          // the state of ansfm_lblrt_set_state; st_n = 0: none
    int st_m0 = -1;                                      // >= 0: the model-by-model loop of a batch is at this model
    int rt_last_rows = 0, rt_last_points = 0, rt_last_chunks = 0;
    // Mie theory over a size distribution (ansfm_mie_makephase): D_n and the series coefficients of a block of radii; inputs,
    // per-thread and per-wavelength state, chunk sums, totals and outputs
    DevBuf mie_ws, mie_st;
    int mie_block = 0, mie_cap = 0;                      // 0: the defaults (kMieBlockDefault radii, 2^20 radii)
    double mie_ms = 0;                                   // kernel time, blocks and the largest block of the last call
    int mie_blocks = 0, mie_block_radii = 0;

    // scattering core: the Hansen walk of g-ordinate g + 1 runs on a second stream beside the chains of g
    hipStream_t ms_stream = nullptr;
    hipStream_t ms_stream2 = nullptr;   // chains of the odd g-ordinates: consecutive chain launches overlap their tails
    hipStream_t ms_stream3 = nullptr;   // G = 1 windows: phase matrices two windows ahead of the chains
    std::vector<hipEvent_t> ms_ev;
    // timing of the last cirsrad call
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double overlap_ms = 0, rt_ms = 0;
    int overlap_launches = 0, rt_launches = 0;

    // the buffers free themselves (DevBuf); streams and events go here
    ~ansfm_ctx()
    {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ms_ev) if (e) (void)hipEventDestroy(e);
        for (hipStream_t s : {ms_stream, ms_stream2, ms_stream3, own_stream}) if (s) (void)hipStreamDestroy(s);
    }
};

#define CHECK_CTX(ctx) do { if (!(ctx)) return ANSFM_ERR_INVALID; } while (0)
#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) {                                                              \
            char b__[512];                                                                    \
            snprintf(b__, sizeof b__, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,           \
                     hipGetErrorString(e__));                                                 \
            ctx->err = b__;                                                                   \
            return ANSFM_ERR_HIP;                                                             \
        }                                                                                     \
    } while (0)
#define FAIL(code, msg) do { ctx->err = (msg); return (code); } while (0)

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
static inline unsigned nblk(size_t n, int b) { return (unsigned)((n + b - 1) / b); }

// length of the register-resident row-head list of the merge kernels: smallest instantiated size >= G
static int merge_list_len(int G)
{
    static const int sizes[] = {8, 10, 16, 20, 32};
    for (int v : sizes) if (v >= G) return v;
    return 32;
}

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
    HIPCHK(ctx->lnK.reserve(total * sizeof(double)));
    HIPCHK(ctx->d_press.reserve(NP * sizeof(double)));
    HIPCHK(ctx->d_temp.reserve(NT * sizeof(double)));
    HIPCHK(ctx->d_wave.reserve((size_t)W * sizeof(double)));
    HIPCHK(ctx->d_delg.reserve(kMaxG * sizeof(double)));
    HIPCHK(ctx->d_flag.reserve(16 * sizeof(int)));
    HIPCHK(hipMemcpyAsync(ctx->d_press.p, PRESS, NP * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_temp.p, TEMP, NT * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_wave.p, WAVE, (size_t)W * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_delg.p, DELG, G * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_flag.p, 0, 16 * sizeof(int), ctx->stream));
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
    ctx->is_lbl = 0; ctx->temp2d = 0;
    ctx->lblrt = 0; ctx->st_n = 0;       // a table replaces a committed line source
    return ANSFM_OK;
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
    HIPCHK(ctx->lnK.reserve(total * sizeof(double)));
    HIPCHK(ctx->d_press.reserve(NP * sizeof(double)));
    HIPCHK(ctx->d_temp.reserve(TEMP.size() * sizeof(double)));                 // [NP][NT] for a table with NT < 0
    HIPCHK(ctx->d_wave.reserve((size_t)W * sizeof(double)));
    HIPCHK(ctx->d_delg.reserve(kMaxG * sizeof(double)));
    HIPCHK(ctx->d_flag.reserve(16 * sizeof(int)));
    HIPCHK(hipMemcpyAsync(ctx->d_press.p, PRESS.data(), NP * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_temp.p, TEMP.data(), TEMP.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_wave.p, WAVE.data(), (size_t)W * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_delg.p, DELG.data(), G * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_flag.p, 0, 16 * sizeof(int), ctx->stream));
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
    ctx->is_lbl = lta ? 1 : 0; ctx->temp2d = (lta && hl.temp2d) ? 1 : 0;
    ctx->lblrt = 0; ctx->st_n = 0;
    if (lta) ctx->monotone = 1;
    ctx->grid_f32 = 1; ctx->delg_f32 = lta ? 0 : 1;   // PRESS / TEMP / DELG come out of the file as float32 arrays (:2544-2559)
    return ANSFM_OK;
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

/* ------------------------------------------------------------------------------------------ */
/* launches                                                                                    */
/* ------------------------------------------------------------------------------------------ */
static int launch_overlap(ansfm_ctx *ctx, bool from_k, const double *kin, int W, int Wpad, int G, int S,
                          int L, int n_models, const LayerInterp *li, const double *amount,
                          const double *del_g_dev, const double *del_g_host, double *tau, bool generic)
{
    // fast path: every k(g) non-decreasing (checked at upload for tables, in the kernel otherwise); generic path:
    // per-lane sort of each gas first (k_ck_overlap<..., SORTED = false>), also on request (the rerun of an unsorted call)
    const bool sorted = !generic && (from_k || ctx->monotone);
    OverlapParams p;
    memset(&p, 0, sizeof p);
    p.lnK = ctx->lnK.as<double>();
    p.kin = kin;
    p.li = li;
    p.amount = amount;
    p.del_g = del_g_dev;
    p.tau = tau;
    p.err_flag = ctx->d_flag.as<int>() + 1;
    p.tile_counter = reinterpret_cast<unsigned int *>(ctx->d_flag.as<int>() + 4);
    HIPCHK(hipMemsetAsync(p.tile_counter, 0, 8 * sizeof(unsigned int), ctx->stream));
    p.W = W; p.Wpad = Wpad; p.G = G; p.NT = ctx->NT; p.S = S; p.L = L; p.n_models = n_models;
    p.delg_f32 = ctx->delg_f32;
    {   // g_ord = [0, cumsum(del_g)], g_ord[ng] = 1 (ForwardModel_0.py:6141-6143); float32 cumsum when DELG is
        double acc = 0.0;
        float accf = 0.0f;
        p.g_ord[0] = 0.0;
        for (int g = 0; g < G; ++g) {
            if (ctx->delg_f32) { accf += (float)del_g_host[g]; p.g_ord[g + 1] = (double)accf; }
            else { acc += del_g_host[g]; p.g_ord[g + 1] = acc; }
        }
        p.g_ord[G] = 1.0;
        p.g_ord[G + 1] = __builtin_nan("");        // never crossed: merge_walk compares with an ordered >=
    }
    // The division-free walk (merge_walk_nodiv) and the 32-bit-key kernel (ansfm_merge32.hip.h, opt-in) need sorted,
    // non-negative input and a first element of the merged order that does not close a bin (rank()'s python [-1] wrap,
    // which only the recorded walk reproduces).  A negative value raises the same flag as an unsorted one in the 32-bit
    // kernel and the call is rerun on the generic path.
    bool nodiv = sorted && G >= 2;
    if (nodiv) {
        const double w00 = ctx->delg_f32 ? (double)((float)del_g_host[0] * (float)del_g_host[0]) : del_g_host[0] * del_g_host[0];
        if (!(w00 < p.g_ord[1])) nodiv = false;
    }
    if (const char *ev = getenv("ANSFM_MERGE_WALK")) { if (!strcmp(ev, "records")) nodiv = false; }
    // a table without a boxed entry is read without the box tests (fast path only; ANSFM_LOAD_BOXTESTS=1 keeps them)
    bool nobox = kLoadNoBox && nodiv && !from_k && !ctx->has_boxed;
    if (const char *ev = getenv("ANSFM_LOAD_BOXTESTS")) { if (ev[0] == '1') nobox = false; }
    bool keys32 = nodiv && ctx->merge_keys == 32;
    if (const char *ev = getenv("ANSFM_MERGE_KEYS")) { keys32 = nodiv && atoi(ev) == 32; }
    const size_t lds = keys32 ? (size_t)overlap32_lds_bytes(G, ctx->delg_f32 != 0)
                              : (size_t)(2 * G + 1) * kWave * sizeof(double) + (size_t)(2 * kMaxG + 2) * sizeof(double) +
                                    kMaxG * sizeof(float) + (sorted ? 0 : (size_t)2 * G * kWave);
    const size_t lds_alloc = (lds + 127) / 128 * 128;      // measured (tools/calib/lds_granule.hip): 7 blocks up to 23 360 bytes
    int per_cu = (int)((160 * 1024) / lds_alloc);
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    if (const char *ev = getenv("ANSFM_WAVES_PER_CU")) { int v = atoi(ev); if (v >= 1 && v < per_cu) per_cu = v; }
    const long ntiles = (long)n_models * (Wpad / kWave) * L;
    long grid = (long)ctx->num_cus * per_cu;
    if (grid > ntiles) grid = ntiles;
    if (grid < 1) grid = 1;
    HIPCHK(ctx->scratch.reserve((size_t)grid * 6 * G * kWave * sizeof(double)));
    p.scratch = ctx->scratch.as<double>();
    if (keys32) {
        HIPCHK(launch_overlap32(p, from_k, merge_list_len(G), (unsigned)grid, ctx->stream));
        return ANSFM_OK;
    }
#define LAUNCH_OV2(D, FK, W32)                                                                                      \
    do {                                                                                                            \
        if (nodiv && nobox)                                                                                         \
            hipLaunchKernelGGL((k_ck_overlap<D, false, W32, true, true, true>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, p); \
        else if (nodiv)                                                                                             \
            hipLaunchKernelGGL((k_ck_overlap<D, FK, W32, true, true>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, p); \
        else if (sorted)                                                                                            \
            hipLaunchKernelGGL((k_ck_overlap<D, FK, W32, true>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, p);  \
        else                                                                                                        \
            hipLaunchKernelGGL((k_ck_overlap<D, FK, W32, false>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, p); \
    } while (0)
#define LAUNCH_OV(D, FK)                                                                              \
    do {                                                                                              \
        if (ctx->delg_f32) LAUNCH_OV2(D, FK, true); else LAUNCH_OV2(D, FK, false);                    \
    } while (0)
#define LAUNCH_OVN(FK)                                                \
    switch (merge_list_len(G)) {                                      \
        case 8: LAUNCH_OV(8, FK); break;                              \
        case 10: LAUNCH_OV(10, FK); break;                            \
        case 16: LAUNCH_OV(16, FK); break;                            \
        case 20: LAUNCH_OV(20, FK); break;                            \
        default: LAUNCH_OV(32, FK); break;                            \
    }
    if (from_k) { LAUNCH_OVN(true); } else { LAUNCH_OVN(false); }
#undef LAUNCH_OVN
#undef LAUNCH_OV
#undef LAUNCH_OV2
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

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

static int launch_rt(ansfm_ctx *ctx, const RtParams &p_in, int n_models)
{
    RtParams p = p_in;
    dim3 grid((unsigned)n_models, (unsigned)p.P, (unsigned)(p.Wpad / kWave));
    if (p.Wpad / kWave > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "thermal RT: more than 65535 wavenumber tiles (4.19e6 wavenumbers)");
    if (p.LIMAX > 1500) FAIL(ANSFM_ERR_UNSUPPORTED, "thermal RT: at most 1500 layers along a path");
    if (p.P > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "thermal RT: at most 65535 paths per call");
    ctx->last_rt_shared = 0;
    // single scattering on the vertical opacities (CIRSrad's branch; the array-level seam hands omega in and keeps the run-time mode)
    const bool ss = p.mode == 2 && p.sca && !p.omega;
    // a de-duplicated batch (the states of a numerical Jacobian) in thermal emission or single scattering: every state starts
    // each path from the record state 0 left after the last layer the two have in common
    static const bool prefix_off = [] { const char *e = getenv("ANSFM_RT_PREFIX"); return e && e[0] == '0'; }();
    const size_t rec = (size_t)p.P * p.LIMAX * 3 * p.G * p.Wpad * sizeof(double);
    if (!prefix_off && n_models >= 4 && n_models <= 65536 && p.tau_slot && (p.mode == 0 || ss) && !p.emi && !p.per_g && rec <= ((size_t)4 << 30)) {
        HIPCHK(ctx->rt_prefix.reserve(rec));
        const size_t nl = (size_t)n_models * p.L * (ss ? p.P : 1), np = (size_t)n_models * p.P;   // ss: flags per path
        const size_t off_j = (nl + 15) & ~(size_t)15;
        HIPCHK(ctx->rt_same.reserve(off_j + np * sizeof(int32_t)));
        unsigned char *same = ctx->rt_same.as<unsigned char>();
        int32_t *jstart = reinterpret_cast<int32_t *>(same + off_j);
        if (ss)
            hipLaunchKernelGGL(k_rt_same_ss, dim3((unsigned)p.L, (unsigned)(n_models - 1)), dim3(256), 0, ctx->stream, p.L, p.Wpad, p.P,
                               p.tau_slot, p.cont, p.sca, p.phase, same);
        else
            hipLaunchKernelGGL(k_rt_same, dim3((unsigned)p.L, (unsigned)(n_models - 1)), dim3(256), 0, ctx->stream, p.L, p.Wpad, p.tau_slot,
                               p.cont_by_row ? nullptr : p.cont, same);      // a continuum stored by row is the row's
        hipLaunchKernelGGL(k_rt_jstart, dim3((unsigned)np), dim3(64), 0, ctx->stream, n_models, p.L, p.P, p.LIMAX, p.nlayin, p.layinc,
                           p.scale, p.emtemp, same, jstart, ss ? 1 : 0);
        p.prefix = ctx->rt_prefix.as<double>(); p.jstart = jstart; p.m0 = 0;
        const size_t lds = (size_t)4 * p.LIMAX * sizeof(double);
        const dim3 g0(1u, grid.y, grid.z), g1((unsigned)(n_models - 1), grid.y, grid.z), blk(kWave, kGY);
        if (ss) {
            hipLaunchKernelGGL((k_thermal_rt<false, 1, true>), g0, blk, lds, ctx->stream, p);
            p.m0 = 1;
            hipLaunchKernelGGL((k_thermal_rt<true, 2, true>), g1, blk, lds, ctx->stream, p);
        } else {
            hipLaunchKernelGGL((k_thermal_rt<false, 1>), g0, blk, lds, ctx->stream, p);
            p.m0 = 1;
            hipLaunchKernelGGL((k_thermal_rt<true, 2>), g1, blk, lds, ctx->stream, p);
        }
        HIPCHK(hipGetLastError());
        ctx->last_rt_shared = 1;
        return ANSFM_OK;
    }
    if (ss && n_models >= 4)
        hipLaunchKernelGGL((k_thermal_rt<true, 0, true>), grid, dim3(kWave, kGY), (size_t)4 * p.LIMAX * sizeof(double), ctx->stream, p);
    else if (ss)
        hipLaunchKernelGGL((k_thermal_rt<false, 0, true>), grid, dim3(kWave, kGY), (size_t)4 * p.LIMAX * sizeof(double), ctx->stream, p);
    else if (n_models >= 4)
        hipLaunchKernelGGL(k_thermal_rt<true>, grid, dim3(kWave, kGY), (size_t)4 * p.LIMAX * sizeof(double), ctx->stream, p);
    else
        hipLaunchKernelGGL(k_thermal_rt<false>, grid, dim3(kWave, kGY), (size_t)4 * p.LIMAX * sizeof(double), ctx->stream, p);
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
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
static int check_unsorted(ansfm_ctx *ctx)
{
    int flag = 0, rc = read_unsorted(ctx, &flag);
    if (rc) return rc;
    if (flag)
        FAIL(ANSFM_ERR_UNSORTED, "k-distribution not non-decreasing in g although the table was flagged monotone at upload");
    return ANSFM_OK;
}

}  // extern "C": the helpers of the entry points below are templates in places

static int launch_overlapg(ansfm_ctx *ctx, bool from_k, const double *kin, const double *dkin, int W, int Wpad, int G, int S,
                           int L, int n_models, const LayerInterp *li, const double *amount, const double *del_g_dev,
                           const double *del_g_host, double *tau, double *dk, bool generic);

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
static int gas_tau(ansfm_ctx *ctx, int n, int L, const double *press, const double *temp, const double *amount, bool generic,
                   double *dk = nullptr)
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
        hipLaunchKernelGGL(k_lblrt_tau, dim3(nblk((size_t)n * L * ctx->Wpad, 256)), dim3(256), 0, ctx->stream, ctx->rt_k.as<double>(),
                           ctx->st_H, ctx->W, ctx->Wpad, ctx->S, L, n, ctx->rt_krow.as<int32_t>() + (size_t)m0 * ctx->S * L, amount,
                           ctx->tau.as<double>(), dk);
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
static int gas_opacity(ansfm_ctx *ctx, int rows, const double *press, const double *temp, const double *amount)
{
    if (!ctx->is_lbl) HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
    int rc = gas_prep(ctx, rows, press, temp);
    if (rc) return rc;
    if (ctx->is_lbl) return gas_tau(ctx, 1, rows, press, temp, amount, false);
    return rerun_unsorted(ctx, [&](bool generic) { return gas_tau(ctx, 1, rows, press, temp, amount, generic); });
}

// Layer de-duplication of a batch of n models x L layers (device rows as above): k_dedup_mark maps every (model, layer) to its
// row in ctx->dd_slot [n][L] -- model 0's L rows first, then the layers in which another model differs (the Rayleigh columns
// ray_totam / ray_f4 take part in the comparison when given) -- the row count is read back (synchronises), and k_dedup_gather
// packs the distinct rows' press, temp [rows] and amount [S][rows] into ctx->dd_in.
struct DedupRows {
    int rows;
    const double *press, *temp, *amount;
};
static int dedup_rows(ansfm_ctx *ctx, int n, int L, const double *press, const double *temp, const double *amount,
                      const double *ray_totam, const double *ray_f4, DedupRows *out)
{
    const int S = ctx->S;
    const size_t nl = (size_t)n * L;
    HIPCHK(ctx->dd_slot.reserve(nl * sizeof(int32_t)));
    HIPCHK(ctx->dd_work.reserve(nl * sizeof(int32_t)));
    int *counter = ctx->d_flag.as<int>() + 12;
    HIPCHK(hipMemsetAsync(counter, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_dedup_mark, dim3(nblk(nl, 128)), dim3(128), 0, ctx->stream, n, L, S, press, temp, amount,
                       ctx->dd_slot.as<int32_t>(), ctx->dd_work.as<int32_t>(), counter, ray_totam, ray_f4);
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

/* ---- host -> device staging of the host-pointer entry points --------------------------------------------------------- */
static int h2d(ansfm_ctx *ctx, DevBuf &b, const void *src, size_t bytes, const void **out)
{
    *out = nullptr;
    if (!src || bytes == 0) return ANSFM_OK;
    HIPCHK(b.reserve(bytes));
    HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    *out = b.p;
    return ANSFM_OK;
}

// The k-th up() of an entry point copies `count` elements into ctx->hb[slot + k] and returns the device copy; a null pointer
// or a zero count gives nullptr.  After an error up() stages nothing more and rc holds its code.  An entry point that stages
// calls no other that stages while its staged pointers are in use.
struct Stager {
    ansfm_ctx *ctx;
    int slot = 0;
    int rc = ANSFM_OK;
    template <class T> const T *up(const T *src, size_t count)
    {
        const void *d = nullptr;
        if (rc == ANSFM_OK) rc = h2d(ctx, ctx->hb[slot++], src, count * sizeof(T), &d);
        return static_cast<const T *>(d);
    }
};

extern "C" {

/* ------------------------------------------------------------------------------------------ */
/* fused CIRSrad (device pointers)                                                             */
/* ------------------------------------------------------------------------------------------ */
// ray_mode: the continuum is Rayleigh scattering alone, of the computed rows (ansfm_cirsrad_ck_thermal_ray_dev); rt_mode 1:
// the path transmission (ansfm_cirsrad_ck_transmission); generic: the merge sorts every k-distribution first (the rerun of a
// call whose table turned out not to be sorted in g)
static int cirsrad_ck_thermal_dev_impl(ansfm_ctx *ctx, int ISPACE, int n_models, int L,
                                 const double *lay_press_pa, const double *lay_temp,
                                 const double *amount, const double *taucont, int P, int LIMAX,
                                 const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                 const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                 const double *SOLFLUX, const double *REFLECTANCE, const double *SOL_ANG,
                                 const double *EMISS_ANG, const double *xfac, double *SPECOUT,
                                 int ray_mode, const double *ray_totam, const double *ray_f4, int rt_mode, bool generic)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsrad: upload a k-table first");
    if (n_models <= 0 || L <= 0 || P <= 0 || LIMAX <= 0 || !lay_press_pa || !lay_temp || !amount || !NLAYIN ||
        !LAYINC || !SCALE || !EMTEMP || !TSURF || !SPECOUT || (ISPACE != 0 && ISPACE != 1))
        FAIL(ANSFM_ERR_INVALID, "cirsrad: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G;
    HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
    // ---- which (model, layer) opacities have to be computed: all of them, or (batches) the distinct ones -------
    DedupRows k{n_models * L, lay_press_pa, lay_temp, amount};   // the rows handed to the merge kernel
    int n_k = n_models;                                         // its view: n_k models of k.rows / n_k layers
    const int32_t *tau_slot = nullptr;
    int rc;
    if (ctx->dedup && n_models > 1 && !ctx->lblrt) {   // the only synchronisation of this entry point (batches only)
        if ((rc = dedup_rows(ctx, n_models, L, lay_press_pa, lay_temp, amount, ray_mode ? ray_totam : nullptr,
                             ray_mode ? ray_f4 : nullptr, &k)))
            return rc;
        n_k = 1;
        tau_slot = ctx->dd_slot.as<int32_t>();
    }
    const int rows = k.rows;
    ctx->last_rows = rows; ctx->last_dedup = tau_slot != nullptr;
    if ((rc = gas_prep(ctx, rows, k.press, k.temp))) return rc;
    const double *cont_t = nullptr;
    if (ray_mode) {
        // the Rayleigh continuum of the rows that are computed (the distinct layers of the batch), straight in the layout the RT
        // reads: the 201 states of a C3 Jacobian have 696 of them, not 20 100
        HIPCHK(ctx->cont_t.reserve((size_t)rows * Wpad * sizeof(double)));
        hipLaunchKernelGGL(k_tau_rayleigh_rows, dim3(nblk((size_t)rows * Wpad, 256)), dim3(256), 0, ctx->stream, rows, W, Wpad, ray_mode,
                           ISPACE, ctx->d_wave.as<double>(), tau_slot ? ctx->dd_work.as<int32_t>() : (const int32_t *)nullptr,
                           ray_totam, ray_f4, ctx->cont_t.as<double>());
        HIPCHK(hipGetLastError());
        cont_t = ctx->cont_t.as<double>();
    } else if (taucont) {
        HIPCHK(ctx->cont_t.reserve((size_t)n_models * L * Wpad * sizeof(double)));
        launch_w_to_last(ctx->stream, (unsigned)n_models, taucont, ctx->cont_t.as<double>(), W, Wpad, 1, L, 0, 0.0, (size_t)W * L, (size_t)L * Wpad);
        HIPCHK(hipGetLastError());
        cont_t = ctx->cont_t.as<double>();
    }
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    if ((rc = gas_tau(ctx, n_k, rows / n_k, k.press, k.temp, k.amount, generic))) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    RtParams r;
    memset(&r, 0, sizeof r);
    r.tau = ctx->tau.as<double>();
    r.tau_slot = tau_slot;
    r.cont = cont_t;
    r.cont_by_row = (ray_mode && tau_slot) ? 1 : 0;
    r.emi = nullptr;
    r.wave = ctx->d_wave.as<double>();
    r.delg = ctx->d_delg.as<double>();
    r.nlayin = NLAYIN; r.layinc = LAYINC; r.scale = SCALE; r.emtemp = EMTEMP;
    r.lay_press = lay_press_pa; r.tsurf = TSURF;
    r.emissivity = EMISSIVITY; r.solflux = SOLFLUX; r.reflectance = REFLECTANCE; r.xfac = xfac;
    r.sol_ang = SOL_ANG; r.emiss_ang = EMISS_ANG;
    r.out = SPECOUT;
    r.W = W; r.Wpad = Wpad; r.G = G; r.L = L; r.P = P; r.LIMAX = LIMAX; r.ispace = ISPACE; r.per_g = 0;
    r.mode = rt_mode;
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
    rc = launch_rt(ctx, r, n_models);
    if (rc != ANSFM_OK) return rc;
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    ctx->overlap_launches = 1;
    ctx->rt_launches = 1;
    ctx->overlap_ms = -1.0;  // resolved lazily in ansfm_last_kernel_ms
    ctx->last_n = n_models; ctx->last_L = L;
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
    return cirsrad_ck_thermal_dev_impl(ctx, ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucont, P, LIMAX, NLAYIN, LAYINC,
                                       SCALE, EMTEMP, TSURF, EMISSIVITY, SOLFLUX, REFLECTANCE, SOL_ANG, EMISS_ANG, xfac, SPECOUT, 0,
                                       nullptr, nullptr, 0, false);
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
    return cirsrad_ck_thermal_dev_impl(ctx, ISPACE, n_models, L, lay_press_pa, lay_temp, amount, nullptr, P, LIMAX, NLAYIN, LAYINC,
                                       SCALE, EMTEMP, TSURF, EMISSIVITY, SOLFLUX, REFLECTANCE, SOL_ANG, EMISS_ANG, xfac, SPECOUT,
                                       ray_mode, TOTAM, ray_mode == 4 ? f4 : nullptr, 0, false);
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
    HIPCHK(ctx->d_flag.reserve(16 * sizeof(int)));
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
static int cirsrad_ck_thermal_host(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                   const double *lay_temp, const double *amount, const double *taucont, int P, int LIMAX,
                                   const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, const double *EMTEMP,
                                   const double *TSURF, const double *EMISSIVITY, const double *SOLFLUX,
                                   const double *REFLECTANCE, const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                                   double *SPECOUT, int rt_mode)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsrad: upload a k-table first");
    if (n_models <= 0 || L <= 0 || P <= 0 || LIMAX <= 0 || !SPECOUT) FAIL(ANSFM_ERR_INVALID, "cirsrad: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, S = ctx->S;
    const size_t D = sizeof(double), nl = (size_t)n_models * L, nlp = (size_t)n_models * LIMAX * P;
    Stager st{ctx};
    const double *press = st.up(lay_press_pa, nl), *temp = st.up(lay_temp, nl), *am = st.up(amount, nl * S),
                 *cont = st.up(taucont, nl * W);
    const int32_t *nlayin = st.up(NLAYIN, P), *layinc = st.up(LAYINC, (size_t)LIMAX * P);
    const double *scale = st.up(SCALE, nlp), *emtemp = st.up(EMTEMP, nlp), *tsurf = st.up(TSURF, n_models),
                 *emis = st.up(EMISSIVITY, W), *solflux = st.up(SOLFLUX, W), *refl = st.up(REFLECTANCE, W),
                 *sol_ang = st.up(SOL_ANG, P), *emiss_ang = st.up(EMISS_ANG, P), *xf = st.up(xfac, W);
    if (st.rc) return st.rc;
    HIPCHK(ctx->tmp_out.reserve((size_t)n_models * W * P * D));
    const int rc = rerun_unsorted(ctx, [&](bool generic) {
        return cirsrad_ck_thermal_dev_impl(ctx, ISPACE, n_models, L, press, temp, am, cont, P, LIMAX, nlayin, layinc, scale, emtemp,
                                           tsurf, emis, solflux, refl, sol_ang, emiss_ang, xf, ctx->tmp_out.as<double>(), 0, nullptr,
                                           nullptr, rt_mode, generic);
    });
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(SPECOUT, ctx->tmp_out.p, (size_t)n_models * W * P * D, hipMemcpyDeviceToHost, ctx->stream));
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
    return cirsrad_ck_thermal_host(ctx, ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucont, P, LIMAX, NLAYIN, LAYINC, SCALE,
                                   EMTEMP, TSURF, EMISSIVITY, SOLFLUX, REFLECTANCE, SOL_ANG, EMISS_ANG, xfac, SPECOUT, 0);
}

int ansfm_cirsrad_ck_transmission(ansfm_ctx *ctx, int n_models, int L, const double *lay_press_pa, const double *lay_temp,
                                  const double *amount, const double *taucont, int P, int LIMAX, const int32_t *NLAYIN,
                                  const int32_t *LAYINC, const double *SCALE, const double *xfac, double *SPECOUT)
{
    CHECK_CTX(ctx);
    if (n_models <= 0 || !SCALE) FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_transmission: bad argument");
    std::vector<double> tsurf((size_t)n_models, -1.0);
    // the emission temperatures are not used by the transmission epilogue: SCALE stands in for the array
    return cirsrad_ck_thermal_host(ctx, 0, n_models, L, lay_press_pa, lay_temp, amount, taucont, P, LIMAX, NLAYIN, LAYINC, SCALE,
                                   SCALE, tsurf.data(), nullptr, nullptr, nullptr, nullptr, nullptr, xfac, SPECOUT, 1);
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

int ansfm_get_dtaugas(ansfm_ctx *ctx, int model, double *dTAUGAS)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table || ctx->dk_n == 0) FAIL(ANSFM_ERR_INVALID, "get_dtaugas: no gradient cirsrad call yet");
    if (model < 0 || model >= ctx->dk_n || !dTAUGAS) FAIL(ANSFM_ERR_INVALID, "get_dtaugas: bad model index");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, L = ctx->dk_L, NP1 = ctx->S + 1;
    const size_t n = (size_t)W * G * NP1 * L;
    HIPCHK(ctx->tmp_out.reserve(n * sizeof(double)));
    hipLaunchKernelGGL(k_dtaugas_to_ref, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream,
                       ctx->dkbuf.as<double>() + (size_t)model * L * NP1 * G * Wpad, ctx->tmp_out.as<double>(), W, Wpad, G, NP1, L);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dTAUGAS, ctx->tmp_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
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
    HIPCHK(ctx->d_flag.reserve(16 * sizeof(int)));
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
    std::vector<int32_t> hi(1 + Li);
    hi[0] = Li;
    for (int j = 0; j < Li; ++j) hi[1 + j] = j;
    std::vector<double> hd(Li + 3, 1.0);
    hd[Li] = TSURF; hd[Li + 1] = SOL_ANG; hd[Li + 2] = EMISS_ANG;
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
static int cirsrad_ck_singlescatt_impl(ansfm_ctx *ctx, const char *fn, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                       const double *lay_temp, const double *amount, const double *taucont, const double *tausca,
                                       const double *phase, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                       const double *SCALE, const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                       const double *BRDF, const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG,
                                       const double *xfac, double *SPECOUT)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) { ctx->err = std::string(fn) + ": upload a k-table first"; return ANSFM_ERR_NOTABLE; }
    bool bad = n_models <= 0 || L <= 0 || P <= 0 || LIMAX <= 0 || !lay_press_pa || !lay_temp || !amount || !tausca || !phase ||
               !NLAYIN || !LAYINC || !SCALE || !EMTEMP || !TSURF || !SOLFLUX || !SOL_ANG || !EMISS_ANG || !SPECOUT ||
               (ISPACE != 0 && ISPACE != 1);
    for (int m = 0; !bad && m < n_models; ++m) bad = TSURF[m] > 0.0 && !EMISSIVITY;
    if (bad) { ctx->err = std::string(fn) + ": bad argument"; return ANSFM_ERR_INVALID; }
    if ((size_t)n_models * P > 65535) { ctx->err = std::string(fn) + ": at most 65535 (model, path) pairs per call"; return ANSFM_ERR_UNSUPPORTED; }
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, S = ctx->S;
    const size_t D = sizeof(double), WL = (size_t)W * L, nl = (size_t)n_models * L, nlp = (size_t)n_models * LIMAX * P;
    Stager st{ctx};
    const double *press = st.up(lay_press_pa, nl), *temp = st.up(lay_temp, nl), *am = st.up(amount, nl * S),
                 *cont = st.up(taucont, n_models * WL), *sca = st.up(tausca, n_models * WL), *ph = st.up(phase, (size_t)n_models * P * WL);
    const int32_t *nlayin = st.up(NLAYIN, P), *layinc = st.up(LAYINC, (size_t)LIMAX * P);
    const double *scale = st.up(SCALE, nlp), *emtemp = st.up(EMTEMP, nlp), *tsurf = st.up(TSURF, n_models),
                 *emis = st.up(EMISSIVITY, W), *brdf = st.up(BRDF, (size_t)W * P), *solflux = st.up(SOLFLUX, W),
                 *sol_ang = st.up(SOL_ANG, P), *emiss_ang = st.up(EMISS_ANG, P), *xf = st.up(xfac, W);
    if (st.rc) return st.rc;
    if (!ctx->is_lbl) HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
    // ---- which (model, layer) opacities have to be computed: all of them, or (batches) the distinct ones -------
    DedupRows k{n_models * L, press, temp, am};
    int n_k = n_models, rc;
    const int32_t *tau_slot = nullptr;
    if (ctx->dedup && n_models > 1 && !ctx->lblrt) {
        if ((rc = dedup_rows(ctx, n_models, L, press, temp, am, nullptr, nullptr, &k))) return rc;
        n_k = 1;
        tau_slot = ctx->dd_slot.as<int32_t>();
    }
    const int rows = k.rows;
    ctx->last_n = n_models; ctx->last_L = L; ctx->last_rows = rows; ctx->last_dedup = tau_slot != nullptr;
    if ((rc = gas_prep(ctx, rows, k.press, k.temp))) return rc;
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (ctx->is_lbl) rc = gas_tau(ctx, n_k, rows / n_k, k.press, k.temp, k.amount, false);
    else rc = rerun_unsorted(ctx, [&](bool generic) { return gas_tau(ctx, n_k, rows / n_k, k.press, k.temp, k.amount, generic); });
    if (rc) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    // reference layouts [n][W][L] -> [n][L][Wpad] (continuum, scattering opacity) and [n][P][W][L] -> [n][P][L][Wpad] (phase)
    const size_t LW = (size_t)L * Wpad;
    HIPCHK(ctx->cont_t.reserve(nl * Wpad * D));
    HIPCHK(ctx->misc.reserve((size_t)n_models * (1 + P) * LW * D));
    double *sca_t = ctx->misc.as<double>(), *ph_t = sca_t + (size_t)n_models * LW;
    const double *cont_t = nullptr;
    if (cont) {
        launch_w_to_last(ctx->stream, (unsigned)n_models, cont, ctx->cont_t.as<double>(), W, Wpad, 1, L, 0, 0.0, WL, LW);
        cont_t = ctx->cont_t.as<double>();
    }
    launch_w_to_last(ctx->stream, (unsigned)n_models, sca, sca_t, W, Wpad, 1, L, 0, 0.0, WL, LW);
    launch_w_to_last(ctx->stream, (unsigned)(n_models * P), ph, ph_t, W, Wpad, 1, L, 0, 0.0, WL, LW);
    HIPCHK(hipGetLastError());
    HIPCHK(ctx->tmp_out.reserve((size_t)n_models * W * P * D));
    RtParams r;
    memset(&r, 0, sizeof r);
    r.tau = ctx->tau.as<double>(); r.tau_slot = tau_slot; r.cont = cont_t; r.sca = sca_t; r.phase = ph_t;
    r.wave = ctx->d_wave.as<double>(); r.delg = ctx->d_delg.as<double>();
    r.nlayin = nlayin; r.layinc = layinc; r.scale = scale;
    r.emtemp = emtemp; r.lay_press = press; r.tsurf = tsurf;
    r.emissivity = emis; r.brdf = brdf; r.solflux = solflux;
    r.sol_ang = sol_ang; r.emiss_ang = emiss_ang; r.xfac = xf;
    r.out = ctx->tmp_out.as<double>();
    r.W = W; r.Wpad = Wpad; r.G = G; r.L = L; r.P = P; r.LIMAX = LIMAX; r.ispace = ISPACE; r.per_g = 0; r.mode = 2;
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
    if ((rc = launch_rt(ctx, r, n_models))) return rc;
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    ctx->overlap_launches = 1; ctx->rt_launches = 1; ctx->overlap_ms = -1.0;
    HIPCHK(hipMemcpyAsync(SPECOUT, ctx->tmp_out.p, (size_t)n_models * W * P * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));      // also: the staged host arrays (TSURF of the single entry) are consumed
    return ANSFM_OK;
}

int ansfm_cirsrad_ck_singlescatt(ansfm_ctx *ctx, int ISPACE, int L, const double *lay_press_pa, const double *lay_temp,
                                 const double *amount, const double *taucont, const double *tausca, const double *phase, int P,
                                 int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                 const double *EMTEMP, double TSURF, const double *EMISSIVITY, const double *BRDF,
                                 const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                                 double *SPECOUT)
{
    return cirsrad_ck_singlescatt_impl(ctx, "cirsrad_ck_singlescatt", ISPACE, 1, L, lay_press_pa, lay_temp, amount, taucont, tausca,
                                       phase, P, LIMAX, NLAYIN, LAYINC, SCALE, EMTEMP, &TSURF, EMISSIVITY, BRDF, SOLFLUX, SOL_ANG,
                                       EMISS_ANG, xfac, SPECOUT);
}

int ansfm_cirsrad_ck_singlescatt_batch(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                       const double *lay_temp, const double *amount, const double *taucont, const double *tausca,
                                       const double *phase, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                       const double *SCALE, const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                       const double *BRDF, const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG,
                                       const double *xfac, double *SPECOUT)
{
    return cirsrad_ck_singlescatt_impl(ctx, "cirsrad_ck_singlescatt_batch", ISPACE, n_models, L, lay_press_pa, lay_temp, amount,
                                       taucont, tausca, phase, P, LIMAX, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, BRDF,
                                       SOLFLUX, SOL_ANG, EMISS_ANG, xfac, SPECOUT);
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
    hipLaunchKernelGGL(k_thermal_emission_g_seam, dim3(nblk(WG, 128)), dim3(128), 0, ctx->stream, ISPACE, W, G, NPAR, NLAYIN, NVMR,
                       wave, tau, dtau, temp, press, TSURF, emis, o_spec, o_dspec, o_dts);
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
    // small path vectors: NLAYIN[1], LAYINC[Li] = identity, SCALE[Li] = 1, TSURF, angles
    std::vector<int32_t> hi(1 + Li);
    hi[0] = Li;
    for (int j = 0; j < Li; ++j) hi[1 + j] = j;
    std::vector<double> hd(Li + 3, 1.0);
    hd[Li] = TSURF; hd[Li + 1] = SOL_ANG; hd[Li + 2] = EMISS_ANG;
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
    r.cont = nullptr;
    r.emi = emi_t;
    r.wave = wave;
    r.delg = nullptr;
    r.nlayin = di;
    r.layinc = di + 1;
    r.scale = dd;
    r.emtemp = temp;
    r.lay_press = press;
    r.tsurf = dd + Li;
    r.emissivity = emis; r.solflux = solflux; r.reflectance = refl;
    r.xfac = nullptr;
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
static int launch_overlapg(ansfm_ctx *ctx, bool from_k, const double *kin, const double *dkin, int W, int Wpad,
                           int G, int S, int L, int n_models, const LayerInterp *li, const double *amount,
                           const double *del_g_dev, const double *del_g_host, double *tau, double *dk, bool generic)
{
    OverlapGParams pg;
    memset(&pg, 0, sizeof pg);
    OverlapParams &p = pg.o;
    p.lnK = ctx->lnK.as<double>();
    p.kin = kin;
    p.li = li;
    p.amount = amount;
    p.del_g = del_g_dev;
    p.tau = tau;
    p.err_flag = ctx->d_flag.as<int>() + 1;
    p.W = W; p.Wpad = Wpad; p.G = G; p.NT = ctx->NT; p.S = S; p.L = L; p.n_models = n_models;
    p.delg_f32 = ctx->delg_f32;
    {
        double acc = 0.0;
        float accf = 0.0f;
        p.g_ord[0] = 0.0;
        for (int g = 0; g < G; ++g) {
            if (ctx->delg_f32) { accf += (float)del_g_host[g]; p.g_ord[g + 1] = (double)accf; }
            else { acc += del_g_host[g]; p.g_ord[g + 1] = acc; }
        }
        p.g_ord[G] = 1.0;
        p.g_ord[G + 1] = __builtin_nan("");        // never crossed: merge_walk compares with an ordered >=
    }
    pg.dkin = dkin;
    pg.dk = dk;
    pg.gas_mask = from_k ? 0xFFFFFFFFu : ctx->grad_gas_mask;      // the array-level seam returns every slot
    const int NP1 = S + 1;
    // the gas selection mask (ansfm_set_gradient_gases) has one bit per gas and bit 31 for temperature
    if (NP1 > 32) FAIL(ANSFM_ERR_UNSUPPORTED, "gradient path supports at most 31 spectroscopic gases");
    // fast path: every k(g) non-decreasing (tables: checked at upload; array-level seam: in the kernel, rerun otherwise)
    const bool sorted = !generic && (from_k || ctx->monotone);
    const size_t lds = (size_t)(2 * G + 1) * kWave * sizeof(double) + (size_t)(2 * kMaxG + 2) * sizeof(double) + kMaxG * sizeof(float) +
                       (sorted ? 0 : (size_t)2 * G * kWave);
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    const long ntiles = (long)n_models * (Wpad / kWave) * L;
    long grid = (long)ctx->num_cus * per_cu;
    if (grid > ntiles) grid = ntiles;
    if (grid < 1) grid = 1;
    HIPCHK(ctx->scratch.reserve((size_t)grid * 6 * (G + 1) * kWave * sizeof(double)));
    HIPCHK(ctx->gscratch.reserve((size_t)grid * (3 + 2 * (size_t)NP1) * G * kWave * sizeof(double)));
    HIPCHK(ctx->perm.reserve((size_t)grid * ((G * G + kCodesPerWord - 1) / kCodesPerWord) * kWave * sizeof(unsigned long long)));
    p.scratch = ctx->scratch.as<double>();
    pg.gscratch = ctx->gscratch.as<double>();
    pg.perm = ctx->perm.as<unsigned long long>();
    p.tile_counter = reinterpret_cast<unsigned int *>(ctx->d_flag.as<int>() + 4);
    HIPCHK(hipMemsetAsync(p.tile_counter, 0, 8 * sizeof(unsigned int), ctx->stream));
#define LAUNCH_OVG(D, FK)                                                                                           \
    do {                                                                                                            \
        if (ctx->delg_f32) {                                                                                        \
            if (sorted) hipLaunchKernelGGL((k_ck_overlapg<D, true, true>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, pg);   \
            else hipLaunchKernelGGL((k_ck_overlapg<D, true, false>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, pg);         \
        } else {                                                                                                    \
            if (sorted) hipLaunchKernelGGL((k_ck_overlapg<D, false, true>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, pg);  \
            else hipLaunchKernelGGL((k_ck_overlapg<D, false, false>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, pg);        \
        }                                                                                                           \
    } while (0)
#define LAUNCH_OVG_D(FK)                                              \
    switch (merge_list_len(G)) {                                      \
        case 8: LAUNCH_OVG(8, FK); break;                             \
        case 10: LAUNCH_OVG(10, FK); break;                           \
        case 16: LAUNCH_OVG(16, FK); break;                           \
        case 20: LAUNCH_OVG(20, FK); break;                           \
        default: LAUNCH_OVG(32, FK); break;                           \
    }
    (void)from_k;                     // the kernel tests p.kin (run-time flag, see load_gas_g)
    LAUNCH_OVG_D(false);
#undef LAUNCH_OVG_D
#undef LAUNCH_OVG
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

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

// transmission: the path transmission and its gradients (ansfm_cirsradg_ck_transmission)
static int cirsradg_ck_thermal_dev_impl(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                        const double *lay_temp, const double *amount, const double *taucont,
                                        const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map_host, int P,
                                        int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                        const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                        const double *xfac, double *SPECOUT, double *dSPECOUT, double *dTSURF, bool transmission)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg: upload a k-table first");
    if (n_models <= 0 || L <= 0 || P <= 0 || LIMAX <= 0 || !lay_press_pa || !lay_temp || !amount || !NLAYIN || !LAYINC ||
        !SCALE || !EMTEMP || !TSURF || !SPECOUT || !dSPECOUT || !dTSURF || !igas_map_host || NPAR <= 0 ||
        NPAR > kMaxPar || NVMR < 0 || NVMR >= NPAR || (ISPACE != 0 && ISPACE != 1))
        FAIL(ANSFM_ERR_INVALID, "cirsradg: bad argument (NPAR <= 256)");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, S = ctx->S, NP1 = S + 1;
    HIPCHK(ctx->dkbuf.reserve((size_t)n_models * L * NP1 * G * Wpad * sizeof(double)));
    HIPCHK(ctx->trold_ws.reserve((size_t)n_models * P * (LIMAX + 1) * G * Wpad * sizeof(double)));
    HIPCHK(ctx->dspec_i.reserve((size_t)n_models * P * NPAR * LIMAX * Wpad * sizeof(double)));
    HIPCHK(hipMemsetAsync(ctx->d_flag.as<int>() + 1, 0, sizeof(int), ctx->stream));
    int rc;
    if ((rc = gas_prep(ctx, n_models * L, lay_press_pa, lay_temp))) return rc;
    const double *cont_t = nullptr, *dcont_t = nullptr;
    if (taucont) {
        HIPCHK(ctx->cont_t.reserve((size_t)n_models * L * Wpad * sizeof(double)));
        launch_w_to_last(ctx->stream, (unsigned)n_models, taucont, ctx->cont_t.as<double>(), W, Wpad, 1, L, 0, 0.0, (size_t)W * L, (size_t)L * Wpad);
        cont_t = ctx->cont_t.as<double>();
    }
    if (dtaucon) {
        HIPCHK(ctx->dcont_t.reserve((size_t)n_models * NPAR * L * Wpad * sizeof(double)));
        launch_w_to_last(ctx->stream, (unsigned)n_models, dtaucon, ctx->dcont_t.as<double>(), W, Wpad, NPAR, L, 0, 0.0, (size_t)W * NPAR * L, (size_t)NPAR * L * Wpad);
        dcont_t = ctx->dcont_t.as<double>();
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    // calc_klblg + :3812-3814 for LBL tables
    if ((rc = gas_tau(ctx, n_models, L, lay_press_pa, lay_temp, amount, false, ctx->dkbuf.as<double>()))) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    RtGParams q;
    memset(&q, 0, sizeof q);
    RtParams &r = q.r;
    r.tau = ctx->tau.as<double>();
    r.cont = cont_t;
    r.wave = ctx->d_wave.as<double>();
    r.delg = ctx->d_delg.as<double>();
    r.nlayin = NLAYIN; r.layinc = LAYINC; r.scale = SCALE; r.emtemp = EMTEMP;
    r.lay_press = lay_press_pa; r.tsurf = TSURF;
    r.emissivity = EMISSIVITY; r.xfac = xfac;
    r.out = SPECOUT;
    r.W = W; r.Wpad = Wpad; r.G = G; r.L = L; r.P = P; r.LIMAX = LIMAX; r.ispace = ISPACE; r.per_g = 0;
    r.mode = transmission ? 1 : 0;
    q.dk = ctx->dkbuf.as<double>();
    q.dcont = dcont_t;
    q.dcont_gas = nullptr;
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
    q.dtsurf = dTSURF;
    q.NPAR = NPAR; q.NVMR = NVMR; q.NP1 = NP1;
    q.gas_mask = ctx->is_lbl ? 0xFFFFFFFFu : ctx->grad_gas_mask;
    for (int k = 0; k < kMaxPar; ++k) q.slot_of_param[k] = -1;
    for (int i = 0; i < S; ++i) {   // assignment order of :3868-3870: a later gas overwrites an earlier one
        if (igas_map_host[i] < 0 || igas_map_host[i] >= NPAR) FAIL(ANSFM_ERR_INVALID, "cirsradg: igas_map out of range");
        // a gas that is not selected leaves the parameter to an earlier selected gas of the same column (isotopologues)
        if ((q.gas_mask >> i) & 1u) q.slot_of_param[igas_map_host[i]] = (signed char)i;
    }
    q.slot_of_param[NVMR] = (q.gas_mask >> 31) ? (signed char)S : (signed char)-1;   // :3872 (written last)
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
    {
        dim3 grid((unsigned)n_models, (unsigned)P, (unsigned)(Wpad / kWave));
        if (Wpad / kWave > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "thermal RT: more than 65535 wavenumber tiles (4.19e6 wavenumbers)");
        // reduction buffer [NP1+2][GY][64] doubles: the largest GY that leaves room for one block per CU
        const size_t per_gy = (size_t)(NP1 + 2) * kWave * sizeof(double);
        if (16 * per_gy <= 128 * 1024)
            hipLaunchKernelGGL(k_thermal_rtg<16>, grid, dim3(kWave, 16), 16 * per_gy, ctx->stream, q);
        else if (8 * per_gy <= 128 * 1024)
            hipLaunchKernelGGL(k_thermal_rtg<8>, grid, dim3(kWave, 8), 8 * per_gy, ctx->stream, q);
        else
            hipLaunchKernelGGL(k_thermal_rtg<4>, grid, dim3(kWave, 4), 4 * per_gy, ctx->stream, q);
        HIPCHK(hipGetLastError());
    }
    for (int m = 0; m < n_models; ++m) {
        const size_t nout = (size_t)W * NPAR * LIMAX * P;
        hipLaunchKernelGGL(k_dspec_to_ref, dim3(nblk(nout, 256)), dim3(256), 0, ctx->stream,
                           ctx->dspec_i.as<double>() + (size_t)m * P * NPAR * LIMAX * Wpad, dSPECOUT + (size_t)m * nout, W,
                           Wpad, NPAR, LIMAX, P, NLAYIN);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    ctx->overlap_launches = 1; ctx->rt_launches = 1;
    ctx->last_n = n_models; ctx->last_L = L;
    return ANSFM_OK;
}

int ansfm_cirsradg_ck_thermal_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                  const double *lay_temp, const double *amount, const double *taucont,
                                  const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map_host, int P,
                                  int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                  const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                  const double *xfac, double *SPECOUT, double *dSPECOUT, double *dTSURF)
{
    return cirsradg_ck_thermal_dev_impl(ctx, ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR,
                                        igas_map_host, P, LIMAX, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, xfac, SPECOUT,
                                        dSPECOUT, dTSURF, false);
}

static int cirsradg_ck_thermal_host(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                    const double *lay_temp, const double *amount, const double *taucont, const double *dtaucon,
                                    int NVMR, int NPAR, const int32_t *igas_map, int P, int LIMAX, const int32_t *NLAYIN,
                                    const int32_t *LAYINC, const double *SCALE, const double *EMTEMP, const double *TSURF,
                                    const double *EMISSIVITY, const double *xfac, double *SPECOUT, double *dSPECOUT,
                                    double *dTSURF, bool transmission)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsradg: upload a k-table first");
    if (n_models <= 0 || L <= 0 || P <= 0 || LIMAX <= 0 || NPAR <= 0 || !SPECOUT || !dTSURF || (!dSPECOUT && n_models != 1))
        FAIL(ANSFM_ERR_INVALID, "cirsradg: bad argument (dSPECOUT may be NULL for a single model: the gradients then stay on the "
                                "device for ansfm_map2pro)");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, S = ctx->S;
    const size_t D = sizeof(double), nl = (size_t)n_models * L, nlp = (size_t)n_models * LIMAX * P;
    Stager st{ctx};
    const double *press = st.up(lay_press_pa, nl), *temp = st.up(lay_temp, nl), *am = st.up(amount, nl * S),
                 *cont = st.up(taucont, nl * W), *dcont = st.up(dtaucon, nl * W * NPAR);
    const int32_t *nlayin = st.up(NLAYIN, P), *layinc = st.up(LAYINC, (size_t)LIMAX * P);
    const double *scale = st.up(SCALE, nlp), *emtemp = st.up(EMTEMP, nlp), *tsurf = st.up(TSURF, n_models),
                 *emis = st.up(EMISSIVITY, W), *xf = st.up(xfac, W);
    if (st.rc) return st.rc;
    const size_t nsp = (size_t)n_models * W * P, ndsp = (size_t)n_models * W * NPAR * LIMAX * P;
    HIPCHK(ctx->tmp_out.reserve((2 * nsp) * D));
    HIPCHK(ctx->dspec_ref.reserve(ndsp * D));     // kept on the device for ansfm_map2pro(dSPECIN = NULL)
    ctx->dspec_dims[0] = 0;
    double *o_spec = ctx->tmp_out.as<double>(), *o_dts = o_spec + nsp;
    const int rc = cirsradg_ck_thermal_dev_impl(ctx, ISPACE, n_models, L, press, temp, am, cont, dcont, NVMR, NPAR, igas_map, P,
                                                LIMAX, nlayin, layinc, scale, emtemp, tsurf, emis, xf, o_spec,
                                                ctx->dspec_ref.as<double>(), o_dts, transmission);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(SPECOUT, o_spec, nsp * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(dTSURF, o_dts, nsp * D, hipMemcpyDeviceToHost, ctx->stream));
    if (dSPECOUT) HIPCHK(hipMemcpyAsync(dSPECOUT, ctx->dspec_ref.p, ndsp * D, hipMemcpyDeviceToHost, ctx->stream));
    if (n_models == 1) { ctx->dspec_dims[0] = ctx->W; ctx->dspec_dims[1] = NPAR; ctx->dspec_dims[2] = LIMAX; ctx->dspec_dims[3] = P; }
    return check_unsorted(ctx);
}

int ansfm_cirsradg_ck_thermal(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                              const double *lay_temp, const double *amount, const double *taucont,
                              const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P, int LIMAX,
                              const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, const double *EMTEMP,
                              const double *TSURF, const double *EMISSIVITY, const double *xfac, double *SPECOUT,
                              double *dSPECOUT, double *dTSURF)
{
    return cirsradg_ck_thermal_host(ctx, ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map,
                                    P, LIMAX, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, xfac, SPECOUT, dSPECOUT, dTSURF,
                                    false);
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
    // no emission in this branch: SCALE stands in for the (unused) emission temperatures, dTSURF is identically zero
    return cirsradg_ck_thermal_host(ctx, 0, n_models, L, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map, P,
                                    LIMAX, NLAYIN, LAYINC, SCALE, SCALE, tsurf.data(), nullptr, xfac, SPECOUT, dSPECOUT, dts.data(),
                                    true);
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
    HIPCHK(ctx->d_flag.reserve(16 * sizeof(int)));
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
        double temp1 = lay_temp[l];
        int it = 0;
        for (int k = 1; k < NT; ++k) if (fabs(cia_temp[k] - temp1) < fabs(cia_temp[it] - temp1)) it = k;
        int itl, ithi;
        if (cia_temp[it] >= temp1) {
            ithi = it;
            if (it == 0) { temp1 = cia_temp[0]; itl = 0; ithi = 1; } else itl = it - 1;
        } else {
            itl = it;
            if (it == NT - 1) { temp1 = cia_temp[it]; ithi = NT - 1; itl = NT - 2; } else ithi = it + 1;
        }
        double frac1 = lay_frac[l];
        int ip = 0;
        for (int k = 1; k < nfrac; ++k) if (fabs(cia_frac[k] - frac1) < fabs(cia_frac[ip] - frac1)) ip = k;
        int ipl, iphi;
        if (cia_frac[ip] >= frac1) {
            iphi = ip;
            if (ip == 0) { frac1 = cia_frac[0]; ipl = 0; iphi = 1; } else ipl = ip - 1;
        } else {
            ipl = ip;
            if (ip == NPARA - 1) { temp1 = cia_frac[ip]; iphi = NPARA - 1; ipl = NPARA - 2; } else iphi = ip + 1;
        }
        if (NPARA == 0) { ipl = 0; iphi = 0; }
        if (ipl < 0 || iphi < 0 || ipl >= NPE || iphi >= NPE || (nfrac > 1 && iphi >= nfrac))
            FAIL(ANSFM_ERR_INVALID, "calc_tau_cia: para-H2 bracket outside K_CIA (the reference raises IndexError here)");
        CiaLayer c;
        c.itl = itl; c.ithi = ithi; c.ipl = ipl; c.iphi = iphi;
        c.fhl_t = (temp1 - cia_temp[itl]) / (cia_temp[ithi] - cia_temp[itl]);
        c.fhh_t = (cia_temp[ithi] - temp1) / (cia_temp[ithi] - cia_temp[itl]);
        c.dfhldT = 1.0 / (cia_temp[ithi] - cia_temp[itl]);
        if (nfrac > 1) {
            c.fhl_f = (frac1 - cia_frac[ipl]) / (cia_frac[iphi] - cia_frac[ipl]);
            c.fhh_f = (cia_frac[iphi] - frac1) / (cia_frac[iphi] - cia_frac[ipl]);
        } else { c.fhl_f = 0.5; c.fhh_f = 0.5; }
        c.xfac = xfac[l];
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
};

// one model's continuum already on the device, [W][L] / [W][ncont][L] (null = zeros): cirsrad_ck_scatter_impl stages none then
struct MsDevCont { const double *cia, *dust, *ray, *sca, *lf; };

static int ms_check(ansfm_ctx *ctx, const MsCall &c, const char *fn)
{
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, std::string(fn) + ": upload a k-table first");
    if (c.n_models <= 0 || c.L <= 0 || !c.lay_press_pa || !c.lay_temp || !c.amount || c.ncont < 0 || c.ngeom <= 0 || c.nmu < 2 ||
        c.nf < 0 || c.nphi <= 0 || !c.radg || !c.sol_angs || !c.emiss_angs || !c.aphis || !c.solar || !c.brdf_matrix || !c.mu1 ||
        !c.wt1 || !c.SPECOUT || (c.ISPACE != 0 && c.ISPACE != 1) || (c.ncont > 0 && (!c.phasarr || !c.lfrac || c.nth < 3)))
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
    const dim3 hg((unsigned)(pp.ncont + (pp.iray > 0 ? 1 : 0))), hb(64);
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

// one model; reuse_walk: ms_single's; dc: its continuum on the device instead of c's host arrays
static int cirsrad_ck_scatter_impl(ansfm_ctx *ctx, const MsCall &c, const MsKnobs &kn, bool reuse_walk, const MsDevCont *dc = nullptr)
{
    int rc = ms_check(ctx, c, "cirsrad_ck_scatter");
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, S = ctx->S, L = c.L;
    MsParams p;
    MsRoute r;
    if ((rc = ms_setup(ctx, p, c, W, G, L, kn, r))) return rc;
    const size_t D = sizeof(double), WL = (size_t)W * L;
    Stager st{ctx};
    const double *press = st.up(c.lay_press_pa, L), *temp = st.up(c.lay_temp, L), *am = st.up(c.amount, (size_t)S * L),
                 *cia = st.up(dc ? nullptr : c.taucia, WL), *dust = st.up(dc ? nullptr : c.taudust, WL),
                 *ray = st.up(dc ? nullptr : c.tauray, WL), *sca = st.up(dc ? nullptr : c.tauscat, WL),
                 *phas = st.up(c.phasarr, (size_t)c.ncont * W * 2 * c.nth), *lf = st.up(dc ? nullptr : c.lfrac, WL * c.ncont),
                 *rg = st.up(c.radg, (size_t)W * c.nmu), *sol = st.up(c.solar, W),
                 *brdf = st.up(c.brdf_matrix, (size_t)W * c.nmu * c.nmu * (c.nf + 1)), *xf = st.up(c.xfac, W);
    if ((rc = st.rc)) return rc;
    if (dc) { cia = dc->cia; dust = dc->dust; ray = dc->ray; sca = dc->sca; lf = dc->lf; }
    // ---- vertical gas opacities: calc_k + k_overlap (:3855-3874), as in the thermal branch --------------------------
    HIPCHK(ctx->ms_taus.reserve(WL * G * D));
    HIPCHK(ctx->ms_omegas.reserve(WL * G * D));
    HIPCHK(ctx->ms_bnu.reserve(WL * D));
    const double *d_tauray = ray;
    if ((rc = ms_zero_tauray(ctx, WL, &d_tauray)) || (rc = gas_opacity(ctx, L, press, temp, am))) return rc;
    ctx->last_n = 1; ctx->last_L = L; ctx->last_rows = L; ctx->last_dedup = 0;
    // ---- TAUTOT, OMEGA, BB -----------------------------------------------------------------------------------------
    MsOpticsParams o;
    memset(&o, 0, sizeof o);
    o.taugas = ctx->tau.as<double>(); o.taucia = cia; o.taudust = dust;
    o.tauray = ray; o.tauscat = sca;
    o.wave = ctx->d_wave.as<double>(); o.lay_temp = temp;
    o.taus = ctx->ms_taus.as<double>(); o.omegas = ctx->ms_omegas.as<double>(); o.bnu = ctx->ms_bnu.as<double>();
    o.W = W; o.Wpad = Wpad; o.G = G; o.L = L; o.ispace = c.ISPACE;
    hipLaunchKernelGGL(k_ms_optics, dim3(nblk((size_t)W, 128), (unsigned)L), dim3(128), 0, ctx->stream, o);
    HIPCHK(hipGetLastError());
    // ---- doubling / adding, g-quadrature ------------------------------------------------------------------------------
    p.phasarr = phas; p.radg = rg; p.solar = sol;
    p.brdf = brdf; p.bnu = o.bnu; p.taus = o.taus; p.tauray = d_tauray; p.omegas = o.omegas;
    p.lfrac = lf;
    if (p.nmu_real && (rc = ms_pad_inputs(ctx, c.nmu, (size_t)W, (size_t)W, c.nf, &p.radg, &p.brdf))) return rc;
    if ((rc = ms_single(ctx, p, r, kn, reuse_walk))) return rc;
    return ms_gquad(ctx, 1, c.ngeom, xf, c.SPECOUT, c.SPEC_G, nullptr);
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
static int cirsrad_ck_scatter_batch_impl(ansfm_ctx *ctx, const MsCall &c, const MsKnobs &kn)
{
    int rc = ms_check(ctx, c, "cirsrad_ck_scatter_batch");
    if (rc) return rc;
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, S = ctx->S, L = c.L, n_models = c.n_models;
    const int ncont = c.ncont, ngeom = c.ngeom, nmu = c.nmu, nf = c.nf, w_begin = c.w_begin;
    const bool sliced = c.W_full != W;
    const size_t D = sizeof(double), WL = (size_t)W * L;
    const bool by_rows = c.cont_row != nullptr;
    const size_t RW = by_rows ? (size_t)c.R * W : 0;
    if (by_rows) {                                              // before anything is launched
        if (c.R <= 0) FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_scatter_batch_rows: R must be positive");
        for (size_t i = 0; i < (size_t)n_models * L; ++i)
            if (c.cont_row[i] < 0 || c.cont_row[i] >= c.R)
                FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_scatter_batch_rows: cont_row[" + std::to_string(i / L) + "][" + std::to_string(i % L) +
                                            "] = " + std::to_string(c.cont_row[i]) + " is outside [0, R = " + std::to_string(c.R) + ")");
    }
    ctx->ms_cache_hits = 0; ctx->ms_cache_layers = (long)n_models * L;
    // (a runtime line source has its own row map, which the (p, T, amount) comparison of the layer cache does not see)
    const bool use_cache = n_models > 1 && ctx->dedup && kn.layer_cache && !ctx->lblrt;      // any stream count
    if (!use_cache && sliced)
        FAIL(ANSFM_ERR_UNSUPPORTED, "cirsrad_ck_scatter_batch_slice: a slice needs the layer cache (n_models > 1, layer de-duplication on)");
    if (!use_cache) {
        // a single model, or de-duplication switched off (ansfm_set_layer_dedup): model by model; m > 0: same phase functions,
        // quadrature, orders -- model 0's walk stands
        // by rows: the rows go up once, behind the staging slots of the single-model entry; a model's dense arrays are formed
        // from them on the device, one model at a time in one buffer
        HIPCHK(hipSetDevice(ctx->device));
        Stager sr{ctx, 14};
        const int32_t *d_crow = by_rows ? sr.up(c.cont_row, (size_t)n_models * L) : nullptr;
        const double *rsrc[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        if (by_rows) {
            rsrc[0] = sr.up(c.taucia, RW); rsrc[1] = sr.up(c.taudust, RW); rsrc[2] = sr.up(c.tauray, RW); rsrc[3] = sr.up(c.tauscat, RW);
            rsrc[4] = sr.up(c.lfrac, RW * ncont);
            if ((rc = sr.rc)) return rc;
            HIPCHK(ctx->ms_tauray_l.reserve((4 + (size_t)ncont) * WL * D));
        }
        for (int m = 0; m < n_models; ++m) {
            const size_t mm = m;
            MsCall cm = c;
            cm.n_models = 1;
            cm.lay_press_pa += mm * L; cm.lay_temp += mm * L; cm.amount += mm * S * L;
            cm.radg += mm * W * nmu; cm.SPECOUT += mm * W * ngeom;
            if (ctx->lblrt) ctx->st_m0 = m;                      // gas_tau reads this model's rows of the state
            if (by_rows) {
                const double *dense[5];
                for (int a = 0; a < 5; ++a) {
                    const int X = a < 4 ? 1 : ncont;
                    double *dst = ctx->ms_tauray_l.as<double>() + (size_t)a * WL;
                    dense[a] = (rsrc[a] && X > 0) ? dst : nullptr;
                    if (dense[a])
                        hipLaunchKernelGGL(k_ms_rows_expand, dim3(nblk((size_t)W, 128), (unsigned)L, (unsigned)X), dim3(128), 0, ctx->stream,
                                           W, X, L, d_crow + mm * L, rsrc[a], dst);
                }
                HIPCHK(hipGetLastError());
                const MsDevCont dc{dense[0], dense[1], dense[2], dense[3], dense[4]};
                rc = cirsrad_ck_scatter_impl(ctx, cm, kn, m > 0, &dc);
                ctx->st_m0 = -1;
                if (rc) return rc;
                continue;
            }
            for (const double **a : {&cm.taucia, &cm.taudust, &cm.tauray, &cm.tauscat}) if (*a) *a += mm * WL;
            if (cm.lfrac) cm.lfrac += mm * WL * ncont;
            rc = cirsrad_ck_scatter_impl(ctx, cm, kn, m > 0);
            ctx->st_m0 = -1;
            if (rc) return rc;
        }
        ctx->last_n = n_models; ctx->last_L = L; ctx->last_rows = n_models * L; ctx->last_dedup = 0;
        return ANSFM_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    MsParams p;
    MsRoute r;
    if ((rc = ms_setup(ctx, p, c, W, G, L, kn, r))) return rc;
    const size_t nl = (size_t)n_models * L;
    const size_t CN = by_rows ? RW : n_models * WL;            // elements of a continuum array: rows, or dense
    Stager st{ctx};
    const double *press = st.up(c.lay_press_pa, nl), *temp = st.up(c.lay_temp, nl), *am = st.up(c.amount, nl * S),
                 *cia = st.up(c.taucia, CN), *dust = st.up(c.taudust, CN), *ray = st.up(c.tauray, CN),
                 *sca = st.up(c.tauscat, CN), *phas = st.up(c.phasarr, (size_t)ncont * c.W_full * 2 * c.nth),
                 *lf = st.up(c.lfrac, CN * ncont), *rg = st.up(c.radg, (size_t)n_models * W * nmu), *sol = st.up(c.solar, W),
                 *brdf = st.up(c.brdf_matrix, (size_t)W * nmu * nmu * (nf + 1)), *xf = st.up(c.xfac, W);
    const int32_t *d_crow = st.up(c.cont_row, by_rows ? nl : 0);
    if ((rc = st.rc)) return rc;
    const double *d_tauray = ray;                               // no TAURAY: every model reads the same zeros
    if (!by_rows && (rc = ms_zero_tauray(ctx, WL, &d_tauray))) return rc;     // (by rows: the optics stage writes the slab's copy)
    // ---- vertical gas opacities of the distinct (model, layer) rows: calc_k + k_overlap ---------------------------------
    DedupRows k;
    if ((rc = dedup_rows(ctx, n_models, L, press, temp, am, nullptr, nullptr, &k)) || (rc = gas_opacity(ctx, k.rows, k.press, k.temp, k.amount)))
        return rc;
    ctx->last_n = n_models; ctx->last_L = L; ctx->last_rows = k.rows; ctx->last_dedup = 1;
    // ---- which layers equal model 0's in EVERY input --------------------------------------------------------------------
    HIPCHK(ctx->ms_same.reserve(nl));
    unsigned char *same = ctx->ms_same.as<unsigned char>();
    if (by_rows)                                                // from the two index maps: no data is compared
        hipLaunchKernelGGL(k_ms_same_index, dim3(nblk(nl, 128)), dim3(128), 0, ctx->stream, n_models, L, ctx->dd_slot.as<int32_t>(), d_crow,
                           same);
    else
        hipLaunchKernelGGL(k_ms_same_init, dim3(nblk(nl, 128)), dim3(128), 0, ctx->stream, n_models, L, ctx->dd_slot.as<int32_t>(), same);
    for (const double *col : {cia, dust, ray, sca})
        if (col && !by_rows)
            hipLaunchKernelGGL(k_ms_same_cols, dim3(nblk((size_t)(n_models - 1) * W, 128)), dim3(128), 0, ctx->stream, n_models, W,
                               1, L, col, same);
    if (lf && ncont > 0 && !by_rows)
        hipLaunchKernelGGL(k_ms_same_cols, dim3(nblk((size_t)(n_models - 1) * W * ncont, 128)), dim3(128), 0, ctx->stream,
                           n_models, W, ncont, L, lf, same);
    HIPCHK(hipGetLastError());
    // where a model's adding sweep may start: below its first changed layer (in sweep order: bottom first when the paths look
    // down, top first when they look up) the stack equals model 0's, kept after every kMsPrefixStep-th layer
    const bool lookup = p.lookup;
    const int npre = L / kMsPrefixStep;
    {
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
                memcmp(c.radg + (size_t)m * W * nmu, c.radg, (size_t)W * nmu * D) != 0)
                lf = 0;
            lstart[m] = std::min(lf / kMsPrefixStep, npre) * kMsPrefixStep;
        }
        // launch order of models 1 .. n-1: by sweep start, so that the blocks of one launch read the same layers of the cache at
        // about the same time (position 0 of the list is unused: model 0 has its own launch)
        std::vector<int> ids((size_t)n_models, 0);
        for (int m = 0; m < n_models; ++m) ids[m] = m;
        std::stable_sort(ids.begin() + 1, ids.end(), [&](int a, int b) { return lstart[a] < lstart[b]; });
        HIPCHK(ctx->ms_lstart.reserve((size_t)2 * n_models * sizeof(int)));
        HIPCHK(hipMemcpyAsync(ctx->ms_lstart.p, lstart.data(), (size_t)n_models * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->ms_lstart.as<int>() + n_models, ids.data(), (size_t)n_models * sizeof(int), hipMemcpyHostToDevice,
                              ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    // ---- phase matrices and Hansen factors: once, they do not depend on the model -----------------------------------------
    p.phasarr = phas; p.radg = rg; p.solar = sol;
    p.brdf = brdf; p.tauray = d_tauray; p.lfrac = lf;
    if (p.nmu_real && (rc = ms_pad_inputs(ctx, nmu, (size_t)n_models * W, (size_t)W, nf, &p.radg, &p.brdf))) return rc;
    const int nmu_k = p.nmu, ncomp = p.ncomp, ncomp_run = r.ncomp_run;    // nmu_k: the stream count the kernels run with
    const size_t nn = (size_t)nmu_k * nmu_k;
    const bool win = G == 1;
    if (!win) {
        // G > 1: the phase matrices of the whole axis and the whole walk in one launch, ahead of the slabs.  The walk continues
        // from g to g + 1 over the whole axis, so a slice walks all of it too: its factors kept, the rest of the steps into a sink
        const size_t per_w = (size_t)(nf + 1) * ncomp * nn, nph = (size_t)c.W_full * per_w, nfc = (size_t)G * W * ncomp * nn;
        const size_t misc_n = 2 * nph + nfc + (sliced ? (size_t)ncomp * nn : 0);
        HIPCHK(ctx->misc.reserve(misc_n * D));
        HIPCHK(hipMemsetAsync(ctx->misc.p, 0, misc_n * D, ctx->stream));
        p.ppl = ctx->misc.as<double>(); p.pmi = p.ppl + nph; p.fc = p.pmi + nph;
        if (ncomp_run > 0) {
            MsParams pw = p;
            pw.nwave = c.W_full; pw.nwin = c.W_full;
            ms_launch_phase(ctx->stream, pw);
            if (sliced) { pw.st0 = w_begin; pw.stn = W; pw.sink = p.fc + nfc; }
            ms_launch_hansen(ctx->stream, pw);
            HIPCHK(hipGetLastError());
        }
        p.ppl += (size_t)w_begin * per_w; p.pmi += (size_t)w_begin * per_w;
    }
    // ---- slabs of the spectral axis sized by the layer cache ----------------------------------------------------------------
    // 16 streams: the cache per wavenumber, and prefix stacks beside it.  Fewer: no prefix stacks (the adding sweep is a few per
    // cent of a chain there), the cache per tile of 64 wavenumbers (the lane kernel's; the wavefront kernel keeps the layout).
    const bool m16 = r.chain == MsChain::mfma16;
    const long unit = m16 ? 1 : 64;
    const size_t entry = m16 ? (size_t)kMsCacheEntry : (2 * (size_t)nmu * nmu + nmu) * 64;  // doubles per (unit, g, order, layer)
    const size_t per_unit = (size_t)G * (nf + 1) * L * entry * D, per_unit_pre = m16 ? (size_t)G * (nf + 1) * npre * entry * D : 0;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    free_b += ctx->ms_cache.bytes + (m16 ? ctx->ms_pcache.bytes : 0);
    const size_t budget = std::min<size_t>(free_b / 2, (size_t)96 << 30);
    long units = (long)(budget / (per_unit + per_unit_pre));
    if (kn.slab) units = std::min(units, (kn.slab + unit - 1) / unit);
    if (units < 1)
        FAIL(ANSFM_ERR_HIP, m16 ? "cirsrad_ck_scatter_batch: no memory for the layer cache of one wavenumber"
                                : "cirsrad_ck_scatter_batch: no memory for the layer cache of one tile of wavenumbers");
    // G = 1: the slabs are the windows of phase matrices and Hansen factors (ms_window_size): a slab's phase matrices and walk
    // -- continuing from the carry of the slab before -- go in front of its chains, model 0's first
    const long Ws = std::min(std::min<long>(W, units * unit), win ? ms_window_size(c.W_full, nf, ncomp, nmu_k, kn) : (long)W);
    ctx->ms_windows = (W + Ws - 1) / Ws; ctx->ms_window_w = Ws;
    if (win) {
        const size_t nph_w = (size_t)Ws * (nf + 1) * ncomp * nn, n_all = 2 * nph_w + (size_t)Ws * ncomp * nn + ncomp * nn;
        HIPCHK(ctx->misc.reserve(n_all * D));
        HIPCHK(hipMemsetAsync(ctx->misc.p, 0, n_all * D, ctx->stream));
        p.ppl = ctx->misc.as<double>(); p.pmi = p.ppl + nph_w; p.fc = p.pmi + nph_w; p.carry = p.fc + (size_t)Ws * ncomp * nn;
        // a slice: the walk of the wavenumbers in front of it, in windows of Ws whose factors only feed the carry
        for (long a = 0; a < w_begin && ncomp_run > 0; a += Ws) {
            MsParams pw = p;
            pw.nwave = c.W_full; pw.pw0 = (int)a; pw.nwin = (int)std::min<long>(Ws, w_begin - a); pw.carry_in = a > 0 ? 1 : 0;
            pw.ig0 = 0; pw.ng_launch = 1;
            ms_launch_phase(ctx->stream, pw);
            ms_launch_hansen(ctx->stream, pw);
            HIPCHK(hipGetLastError());
        }
    }
    const int mchunk = std::min(n_models - 1, kn.chunk ? kn.chunk : 64);
    HIPCHK(ctx->ms_cache.reserve((size_t)((Ws + unit - 1) / unit) * per_unit));
    if (m16) {
        HIPCHK(ctx->ms_pcache.reserve(std::max<size_t>((size_t)Ws * per_unit_pre, 8)));
        HIPCHK(ctx->ms_orders.reserve((size_t)Ws * G * sizeof(int)));
    }
    const size_t opt_models = (size_t)std::max(1, mchunk);
    HIPCHK(ctx->ms_taus.reserve(opt_models * Ws * G * L * D));
    HIPCHK(ctx->ms_omegas.reserve(opt_models * Ws * G * L * D));
    HIPCHK(ctx->ms_bnu.reserve(opt_models * Ws * L * D));
    if (by_rows) {
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
    p.st_wl = ray ? WL : 0; p.st_wcl = (size_t)W * ncont * L; p.st_wm = (size_t)W * nmu_k; p.st_rad = (size_t)ngeom * G * W;
    p.ig0 = 0; p.ng_launch = G;
    MsOpticsRowsParams orw;
    memset(&orw, 0, sizeof orw);
    orw.taugas = ctx->tau.as<double>(); orw.slot = ctx->dd_slot.as<int32_t>(); orw.cont_row = d_crow;
    orw.taucia = cia; orw.taudust = dust; orw.tauray = ray; orw.tauscat = sca; orw.lfrac = lf;
    orw.wave = ctx->d_wave.as<double>(); orw.lay_temp = temp;
    orw.taus = ctx->ms_taus.as<double>(); orw.omegas = ctx->ms_omegas.as<double>(); orw.bnu = ctx->ms_bnu.as<double>();
    orw.tauray_l = ctx->ms_tauray_l.as<double>(); orw.lfrac_l = ctx->ms_lfrac_l.as<double>();
    orw.W = W; orw.Wpad = Wpad; orw.G = G; orw.L = L; orw.ncont = lf ? ncont : 0; orw.ispace = c.ISPACE;
    MsOpticsBatchParams o;
    memset(&o, 0, sizeof o);
    o.taugas = ctx->tau.as<double>(); o.slot = ctx->dd_slot.as<int32_t>();
    o.taucia = cia; o.taudust = dust; o.tauray = ray; o.tauscat = sca;
    o.wave = ctx->d_wave.as<double>(); o.lay_temp = temp;
    o.taus = ctx->ms_taus.as<double>(); o.omegas = ctx->ms_omegas.as<double>(); o.bnu = ctx->ms_bnu.as<double>();
    o.W = W; o.Wpad = Wpad; o.G = G; o.L = L; o.ispace = c.ISPACE;
    // TAUTOT, OMEGA, BB (by rows: and the slab's TAURAY / fractions) of the models [m0, m0 + nm) of the launch order on the slab
    auto optics = [&](int w0, int wc, int m0, int nm, const int *ids) {
        const dim3 grid(nblk((size_t)wc, 128), (unsigned)L, (unsigned)nm);
        if (by_rows) {
            orw.w0 = w0; orw.wcount = wc; orw.m0 = m0; orw.nm = nm; orw.model_ids = ids;
            hipLaunchKernelGGL(k_ms_optics_rows, grid, dim3(128), 0, ctx->stream, orw);
        } else {
            o.w0 = w0; o.wcount = wc; o.m0 = m0; o.nm = nm; o.model_ids = ids;
            hipLaunchKernelGGL(k_ms_optics_batch, grid, dim3(128), 0, ctx->stream, o);
        }
    };
    for (long w0 = 0; w0 < W; w0 += Ws) {
        const int wc = (int)std::min<long>(Ws, W - w0);
        if (win) {
            // the phase matrices of the slab are those of the wavenumbers w_begin + [w0, w0 + wc) of phasarr; chains and walk
            // index the window relative to w0
            p.pw0 = (int)w0; p.nwin = wc; p.carry_in = w_begin + w0 > 0 ? 1 : 0;
            p.ig0 = 0; p.ng_launch = 1;
            if (ncomp_run > 0) {
                MsParams pw = p;
                pw.nwave = c.W_full; pw.pw0 = w_begin + (int)w0;
                ms_launch_phase(ctx->stream, pw);
                ms_launch_hansen(ctx->stream, p);
            }
            HIPCHK(hipGetLastError());
        }
        p.w0 = (int)w0; p.wcount = wc;
        if (by_rows) { p.st_wl = (size_t)wc * L; p.st_wcl = (size_t)wc * ncont * L; }       // between launch positions
        // model 0: the ordinary chain, which also fills the cache
        optics((int)w0, wc, 0, 1, nullptr);
        p.m0 = 0; p.n_launch = 1;
        if ((rc = ms_launch_chain<1>(ctx, r.chain, ctx->stream, p))) return rc;
        // models 1 .. n-1 in chunks: the adding sweep over cached layers, changed layers computed in place
        for (int m0 = 1; m0 < n_models; m0 += mchunk) {
            const int nm = std::min(mchunk, n_models - m0);
            optics((int)w0, wc, m0, nm, p.model_ids);
            p.m0 = m0; p.n_launch = nm;
            if ((rc = ms_launch_chain<2>(ctx, r.chain, ctx->stream, p))) return rc;
        }
    }
    // below 16 streams every Fourier order was worked through: k_ms_fourier applies the reference's convergence break per model
    return ms_gquad(ctx, n_models, ngeom, xf, c.SPECOUT, nullptr, m16 ? nullptr : &p);
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
    const MsCall c{ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucia, taudust, tauray, tauscat, ncont, nth, phasarr,
                   lfrac, radg, ngeom, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, nmu, mu1, wt1, nf, nphi, iray,
                   imie, xfac, SPECOUT, nullptr, ctx->W, 0};
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
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsrad_ck_scatter_batch_slice: upload a k-table first");
    if (w_begin < 0 || (long)w_begin + ctx->W > (long)W_full || (ncont > 0 && !phasarr))
        FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_scatter_batch_slice: the table is not a slice [w_begin, w_begin + W) of W_full, or no phasarr");
    const MsCall c{ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucia, taudust, tauray, tauscat, ncont, nth, phasarr,
                   lfrac, radg, ngeom, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, nmu, mu1, wt1, nf, nphi, iray,
                   imie, xfac, SPECOUT, nullptr, W_full, w_begin};
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
    if (!ctx->have_table) FAIL(ANSFM_ERR_NOTABLE, "cirsrad_ck_scatter_batch_rows: upload a k-table first");
    if (!cont_row || w_begin < 0 || (long)w_begin + ctx->W > (long)W_full || (ncont > 0 && !phasarr))
        FAIL(ANSFM_ERR_INVALID, "cirsrad_ck_scatter_batch_rows: no cont_row, the table is not a slice [w_begin, w_begin + W) of W_full, or no phasarr");
    const MsCall c{ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucia_rows, taudust_rows, tauray_rows, tauscat_rows, ncont,
                   nth, phasarr, lfrac_rows, radg, ngeom, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, nmu, mu1, wt1, nf,
                   nphi, iray, imie, xfac, SPECOUT, nullptr, W_full, w_begin, R, cont_row};
    return cirsrad_ck_scatter_batch_impl(ctx, c, MsKnobs());
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


/* ------------------------------------------------------------------------------------------ */
/* runtime line-by-line                                                                        */
/* ------------------------------------------------------------------------------------------ */
} // extern "C"

static int lbl_shape_built(ansfm_ctx *ctx, int lineshape_id)
{
    if (lineshape_id != 0 && lineshape_id != 4 && lineshape_id != 12)
        FAIL(ANSFM_ERR_UNSUPPORTED, "lineshape: VOIGT (0), LORENTZ (4), DOPPLER (12) are built");   // enum map raises NotImplementedError
    return ANSFM_OK;
}

static int lbl_grid_ascending(ansfm_ctx *ctx, int nw, const double *wn_grid)
{
    for (int j = 1; j < nw; ++j)
        if (wn_grid[j] < wn_grid[j - 1]) FAIL(ANSFM_ERR_INVALID, "wn_grid must be ascending (LineData_0.py:230)");
    return ANSFM_OK;
}

// Lines sorted by wavenumber for the windowed gather (the reference accepts any order; summation order then differs from it
// only in rounding): h = nu, sw, e_lower, stim_ref [N], bparams [3M][N] in sorted order, ord[i] = the caller's index of line i
static void lbl_pack_lines(int M, int N, const double *broadening_params, const double *nu, const double *sw,
                           const double *e_lower, const double *stim_ref, std::vector<int> &ord, std::vector<double> &h)
{
    ord.resize(N);
    for (int i = 0; i < N; ++i) ord[i] = i;
    bool sorted = true;
    for (int i = 1; i < N; ++i) if (nu[i] < nu[i - 1]) { sorted = false; break; }
    if (!sorted) std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return nu[a] < nu[b]; });
    h.resize((size_t)(4 + 3 * M) * N);
    double *hnu = h.data(), *hsw = hnu + N, *hel = hsw + N, *hsr = hel + N, *hbp = hsr + N;
    for (int i = 0; i < N; ++i) {
        const int o = ord[i];
        hnu[i] = nu[o]; hsw[i] = sw[o]; hel[i] = e_lower[o]; hsr[i] = stim_ref[o];
        for (int r = 0; r < 3 * M; ++r) hbp[(size_t)r * N + i] = broadening_params[(size_t)r * N + o];
    }
}

// The geometry of the pseudo-continuum bins on a grid, with the reference's expressions: first / last (:399-416), the largest
// touched grid point (j_max :463; the touched points of a bin are a run, because (wn - c)/w does not decrease along an
// ascending grid), the lower edges and the largest width
struct PcGeometry {
    std::vector<double> lo;
    int first = -1, last = -1, jmax = 0;
    double wmax = 0.0;
};
static int lbl_pc_geometry(ansfm_ctx *ctx, int nw, const double *h_grid, int N, const double *centers, const double *widths,
                           PcGeometry &g)
{
    g.lo.resize(N);
    for (int i = 0; i < N; ++i) {
        const double c = centers[i], w = widths[i];
        if (!(w > 0.0)) FAIL(ANSFM_ERR_INVALID, "pseudo-continuum: bin widths must be positive");
        const double bin_min = c - w / 2.0, bin_max = c + w / 2.0;
        if (i > 0 && !(bin_min >= g.lo[i - 1]))
            FAIL(ANSFM_ERR_INVALID, "pseudo-continuum: the lower bin edges centre - width / 2 must be ascending");
        g.lo[i] = bin_min;
        if (g.first == -1 && bin_min <= h_grid[0]) g.first = i;
        if (g.last == -1 && bin_max > h_grid[nw - 1]) g.last = i;
        if (w > g.wmax) g.wmax = w;
        int a = 0, b = nw;      // first j with (wn_j - c)/w >= 0.5
        while (a < b) { const int mid = (a + b) >> 1; if ((h_grid[mid] - c) / w < 0.5) a = mid + 1; else b = mid; }
        if (a > 0 && (h_grid[a - 1] - c) / w >= -0.5 && a - 1 > g.jmax) g.jmax = a - 1;
    }
    if (g.first == -1) g.first = N;
    if (g.last == -1) g.last = N;
    return ANSFM_OK;
}

// The lines of one isotopologue onto d_out[L][nw] in HBM.  d_grid / d_t / d_p: device copies of the grid and the (T, p)
// points (h_p: the pressures on the host); everything else is staged here, from st's next slot on.  Arguments are checked.
static int lbl_lines_dev(ansfm_ctx *ctx, Stager &st, int nw, const double *d_grid, int lineshape_id, int L, const double *d_t,
                         double t_ref, const double *d_p, const double *h_p, double p_ref, const double *q_ratio,
                         double isotopic_abundance, double isotopic_mass, int M, const double *mol_mix_frac, int N,
                         const double *broadening_params, const double *nu, const double *sw, const double *e_lower,
                         const double *stim_ref, double *d_out, double *store, double s_floor, double wn_calc_window,
                         double wn_approx_window)
{
    std::vector<int> ord;
    std::vector<double> h;
    lbl_pack_lines(M, N, broadening_params, nu, sw, e_lower, stim_ref, ord, h);
    double dmax = 0.0;
    for (int o = 0; o < N; ++o) {
        double d = 0.0;
        for (int j = 0; j < M; ++j) d += fabs(broadening_params[(size_t)(3 * j + 2) * N + o] * mol_mix_frac[j]);
        if (d > dmax) dmax = d;
    }
    double pmax = 0.0;
    for (int l = 0; l < L; ++l) if (fabs(h_p[l] / p_ref) > pmax) pmax = fabs(h_p[l] / p_ref);
    const size_t D = sizeof(double);
    LblParams p;
    memset(&p, 0, sizeof p);
    const double *dl = st.up(h.data(), h.size());
    p.mmf = st.up(mol_mix_frac, M);
    p.q_ratio = st.up(q_ratio, L);
    if (st.rc) return st.rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));   // h is a local buffer
    HIPCHK(ctx->misc.reserve((size_t)L * (kLblRows + 1) * N * D));
    p.wn_grid = d_grid; p.t_calc = d_t; p.p_calc = d_p; p.out = d_out;
    p.nu = dl; p.sw = dl + N; p.e_lower = dl + 2 * (size_t)N; p.stim_ref = dl + 3 * (size_t)N; p.bparams = dl + 4 * (size_t)N;
    p.store = ctx->misc.as<double>();
    p.shift = p.store + (size_t)L * kLblRows * N;
    p.nw = nw; p.N = N; p.M = M; p.L = L; p.lineshape_id = lineshape_id;
    p.t_ref = t_ref; p.p_ref = p_ref; p.iso_abundance = isotopic_abundance; p.iso_mass = isotopic_mass; p.s_floor = s_floor;
    p.wn_calc_window = wn_calc_window; p.wn_approx_window = wn_approx_window;
    p.max_shift = dmax * pmax * 1.0000001 + 1e-12;
    hipLaunchKernelGGL(k_lbl_line_params, dim3(nblk((size_t)L * N, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_lbl_accumulate, dim3(nblk(nw, 256 * kLblPts), (unsigned)L), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    if (store) {   // store[L][4][N] = strength, alpha_d, gamma_l, shift in the caller's line order
        std::vector<double> hst((size_t)L * (kLblRows + 1) * N);
        HIPCHK(hipMemcpyAsync(hst.data(), p.store, hst.size() * D, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        static const int src[3] = {0, 6, 7};
        const double *hsh = hst.data() + (size_t)L * kLblRows * N;
        for (int l = 0; l < L; ++l)
            for (int i = 0; i < N; ++i) {
                const double *rec = hst.data() + ((size_t)l * N + i) * kLblRows;
                for (int r = 0; r < 3; ++r) store[((size_t)l * 4 + r) * N + ord[i]] = rec[src[r]];
                store[((size_t)l * 4 + 3) * N + ord[i]] = hsh[(size_t)l * N + i];
            }
    }
    return ANSFM_OK;
}

// The pseudo-continuum of one isotopologue onto d_out[L][nw] in HBM; h_grid: the grid on the host, for the bin geometry.
static int lbl_pc_dev(ansfm_ctx *ctx, Stager &st, int nw, const double *d_grid, const double *h_grid, int lineshape_id, int L,
                      const double *d_t, double t_ref, const double *d_p, double p_ref, const double *q_ratio,
                      double isotopic_abundance, double isotopic_mass, int M, const double *mol_mix_frac, int N,
                      const double *bparams, const double *centers, const double *widths, const double *sw_sum,
                      const double *e_lower, double *d_out, double *store, double *store_x, int nb)
{
    PcGeometry g;
    const int grc = lbl_pc_geometry(ctx, nw, h_grid, N, centers, widths, g);
    if (grc) return grc;
    const std::vector<double> &lo = g.lo;
    const int first = g.first, last = g.last, jmax = g.jmax;
    const double wmax = g.wmax;
    const size_t D = sizeof(double), LN = (size_t)L * N;
    PcParams p;
    memset(&p, 0, sizeof p);
    p.centers = st.up(centers, N); p.widths = st.up(widths, N); p.sw = st.up(sw_sum, N); p.e_lower = st.up(e_lower, N);
    p.lo = st.up(lo.data(), N); p.bparams = st.up(bparams, (size_t)3 * M * N);
    p.mmf = st.up(mol_mix_frac, M); p.q_ratio = st.up(q_ratio, L);
    if (st.rc) return st.rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));   // lo is a local buffer
    HIPCHK(ctx->misc.reserve(LN * (size_t)(3 + (2 * nb + 1) + 2) * D));
    p.wn_grid = d_grid; p.t_calc = d_t; p.p_calc = d_p; p.out = d_out;
    p.store = ctx->misc.as<double>();
    p.x = p.store + 3 * LN; p.ysum = p.x + LN; p.y = p.ysum + LN;
    p.nw = nw; p.N = N; p.M = M; p.L = L; p.lineshape_id = lineshape_id; p.nb = nb;
    p.first = first; p.last = last; p.jmax = jmax;
    p.t_ref = t_ref; p.p_ref = p_ref; p.iso_abundance = isotopic_abundance; p.iso_mass = isotopic_mass; p.wmax = wmax;
    hipLaunchKernelGGL(k_pc_params, dim3(nblk(LN, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pc_shapes, dim3(nblk(LN, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pc_gather, dim3(nblk(LN, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    if (jmax > 0) {
        hipLaunchKernelGGL(k_pc_interp, dim3(nblk((size_t)jmax, 256), nblk((size_t)L, kPcLayers)), dim3(256), 0, ctx->stream, p);
        HIPCHK(hipGetLastError());
    }
    if (store) HIPCHK(hipMemcpyAsync(store, p.store, 3 * LN * D, hipMemcpyDeviceToHost, ctx->stream));
    if (store_x) HIPCHK(hipMemcpyAsync(store_x, p.x, LN * D, hipMemcpyDeviceToHost, ctx->stream));
    if (store || store_x) HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

static int lbl_pc_args(ansfm_ctx *ctx, int lineshape_id, int M, int N, const double *q_ratio, const double *mol_mix_frac,
                       const double *bparams, const double *centers, const double *widths, const double *sw_sum,
                       const double *e_lower, int nb)
{
    if (M <= 0 || N < 0 || nb < 0 || !q_ratio || !mol_mix_frac || (N > 0 && (!bparams || !centers || !widths || !sw_sum || !e_lower)))
        FAIL(ANSFM_ERR_INVALID, "add_pseudo_continuum_monochromatic_absorption: bad argument");
    if (nb > kPcMaxNeighbours) FAIL(ANSFM_ERR_UNSUPPORTED, "pseudo-continuum: n_neighbour_bins 0 .. 8 are built");
    return lbl_shape_built(ctx, lineshape_id);
}

extern "C" {

int ansfm_add_line_set_monochromatic_absorption(
    ansfm_ctx *ctx, int nw, const double *wn_grid, int lineshape_id, int L, const double *t_calc, double t_ref,
    const double *p_calc, double p_ref, const double *q_ratio, double isotopic_abundance, double isotopic_mass, int M,
    const double *mol_mix_frac, int N, const double *broadening_params, const double *nu, const double *sw,
    const double *e_lower, const double *stim_ref, double *out, double *store, double s_floor, double wn_calc_window,
    double wn_approx_window)
{
    CHECK_CTX(ctx);
    if (nw <= 0 || L <= 0 || M <= 0 || N < 0 || !wn_grid || !t_calc || !p_calc || !q_ratio || !mol_mix_frac || !out ||
        (N > 0 && (!broadening_params || !nu || !sw || !e_lower || !stim_ref)))
        FAIL(ANSFM_ERR_INVALID, "add_line_set_monochromatic_absorption: bad argument");
    int rc = lbl_shape_built(ctx, lineshape_id);
    if (rc || (rc = lbl_grid_ascending(ctx, nw, wn_grid))) return rc;
    if (N == 0) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Stager st{ctx};
    const double *d_grid = st.up(wn_grid, nw), *d_t = st.up(t_calc, L), *d_p = st.up(p_calc, L);
    double *d_out = const_cast<double *>(st.up(out, (size_t)L * nw));     // accumulated onto
    if (st.rc) return st.rc;
    rc = lbl_lines_dev(ctx, st, nw, d_grid, lineshape_id, L, d_t, t_ref, d_p, p_calc, p_ref, q_ratio, isotopic_abundance,
                       isotopic_mass, M, mol_mix_frac, N, broadening_params, nu, sw, e_lower, stim_ref, d_out, store, s_floor,
                       wn_calc_window, wn_approx_window);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)L * nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_add_pseudo_continuum_monochromatic_absorption(
    ansfm_ctx *ctx, int nw, const double *wn_grid, int lineshape_id, int L, const double *t_calc, double t_ref,
    const double *p_calc, double p_ref, const double *q_ratio, double isotopic_abundance, double isotopic_mass, int M,
    const double *mol_mix_frac, int N, const double *lsw_mean_broadening_params, const double *wn_bin_centers,
    const double *wn_bin_widths, const double *sw_sum, const double *lsw_mean_e_lower, double *out, double *store,
    double *store_x, int n_neighbour_bins)
{
    CHECK_CTX(ctx);
    if (nw <= 0 || L <= 0 || !wn_grid || !t_calc || !p_calc || !out)
        FAIL(ANSFM_ERR_INVALID, "add_pseudo_continuum_monochromatic_absorption: bad argument");
    int rc = lbl_pc_args(ctx, lineshape_id, M, N, q_ratio, mol_mix_frac, lsw_mean_broadening_params, wn_bin_centers,
                         wn_bin_widths, sw_sum, lsw_mean_e_lower, n_neighbour_bins);
    if (rc || (rc = lbl_grid_ascending(ctx, nw, wn_grid))) return rc;
    if (N == 0) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Stager st{ctx};
    const double *d_grid = st.up(wn_grid, nw), *d_t = st.up(t_calc, L), *d_p = st.up(p_calc, L);
    double *d_out = const_cast<double *>(st.up(out, (size_t)L * nw));     // accumulated onto
    if (st.rc) return st.rc;
    rc = lbl_pc_dev(ctx, st, nw, d_grid, wn_grid, lineshape_id, L, d_t, t_ref, d_p, p_ref, q_ratio, isotopic_abundance,
                    isotopic_mass, M, mol_mix_frac, N, lsw_mean_broadening_params, wn_bin_centers, wn_bin_widths, sw_sum,
                    lsw_mean_e_lower, d_out, store, store_x, n_neighbour_bins);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)L * nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

/* ---- the opacity of a gas in HBM: the sum over its isotopologues of lines and pseudo-continuum -------------------------- */
int ansfm_lbl_accum_begin(ansfm_ctx *ctx, int nw, const double *wn_grid, int L, const double *t_calc, const double *p_calc)
{
    CHECK_CTX(ctx);
    ctx->acc_nw = ctx->acc_L = 0;
    if (nw <= 0 || L <= 0 || !wn_grid || !t_calc || !p_calc) FAIL(ANSFM_ERR_INVALID, "lbl_accum_begin: bad argument");
    const int rc = lbl_grid_ascending(ctx, nw, wn_grid);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double);
    HIPCHK(ctx->acc.reserve((size_t)L * nw * D));
    HIPCHK(ctx->acc_grid.reserve((size_t)nw * D));
    HIPCHK(ctx->acc_tp.reserve((size_t)2 * L * D));
    ctx->acc_h_grid.assign(wn_grid, wn_grid + nw);
    ctx->acc_h_p.assign(p_calc, p_calc + L);
    HIPCHK(hipMemsetAsync(ctx->acc.p, 0, (size_t)L * nw * D, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->acc_grid.p, ctx->acc_h_grid.data(), (size_t)nw * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->acc_tp.p, t_calc, (size_t)L * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->acc_tp.as<double>() + L, p_calc, (size_t)L * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // t_calc / p_calc are the caller's
    ctx->acc_nw = nw; ctx->acc_L = L;
    return ANSFM_OK;
}

int ansfm_lbl_accum_add_lines(ansfm_ctx *ctx, int lineshape_id, double t_ref, double p_ref, const double *q_ratio,
                              double isotopic_abundance, double isotopic_mass, int M, const double *mol_mix_frac, int N,
                              const double *broadening_params, const double *nu, const double *sw, const double *e_lower,
                              const double *stim_ref, double *store, double s_floor, double wn_calc_window,
                              double wn_approx_window)
{
    CHECK_CTX(ctx);
    if (ctx->acc_nw <= 0) FAIL(ANSFM_ERR_INVALID, "lbl_accum_add_lines: call ansfm_lbl_accum_begin first");
    if (M <= 0 || N < 0 || !q_ratio || !mol_mix_frac || (N > 0 && (!broadening_params || !nu || !sw || !e_lower || !stim_ref)))
        FAIL(ANSFM_ERR_INVALID, "lbl_accum_add_lines: bad argument");
    const int rc = lbl_shape_built(ctx, lineshape_id);
    if (rc) return rc;
    if (N == 0) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Stager st{ctx};
    const int L = ctx->acc_L;
    return lbl_lines_dev(ctx, st, ctx->acc_nw, ctx->acc_grid.as<double>(), lineshape_id, L, ctx->acc_tp.as<double>(), t_ref,
                         ctx->acc_tp.as<double>() + L, ctx->acc_h_p.data(), p_ref, q_ratio, isotopic_abundance, isotopic_mass, M,
                         mol_mix_frac, N, broadening_params, nu, sw, e_lower, stim_ref, ctx->acc.as<double>(), store, s_floor,
                         wn_calc_window, wn_approx_window);
}

int ansfm_lbl_accum_add_pseudo_continuum(ansfm_ctx *ctx, int lineshape_id, double t_ref, double p_ref, const double *q_ratio,
                                         double isotopic_abundance, double isotopic_mass, int M, const double *mol_mix_frac,
                                         int N, const double *lsw_mean_broadening_params, const double *wn_bin_centers,
                                         const double *wn_bin_widths, const double *sw_sum, const double *lsw_mean_e_lower,
                                         double *store, double *store_x, int n_neighbour_bins)
{
    CHECK_CTX(ctx);
    if (ctx->acc_nw <= 0) FAIL(ANSFM_ERR_INVALID, "lbl_accum_add_pseudo_continuum: call ansfm_lbl_accum_begin first");
    const int rc = lbl_pc_args(ctx, lineshape_id, M, N, q_ratio, mol_mix_frac, lsw_mean_broadening_params, wn_bin_centers,
                               wn_bin_widths, sw_sum, lsw_mean_e_lower, n_neighbour_bins);
    if (rc) return rc;
    if (N == 0) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Stager st{ctx};
    const int L = ctx->acc_L;
    return lbl_pc_dev(ctx, st, ctx->acc_nw, ctx->acc_grid.as<double>(), ctx->acc_h_grid.data(), lineshape_id, L,
                      ctx->acc_tp.as<double>(), t_ref, ctx->acc_tp.as<double>() + L, p_ref, q_ratio, isotopic_abundance,
                      isotopic_mass, M, mol_mix_frac, N, lsw_mean_broadening_params, wn_bin_centers, wn_bin_widths, sw_sum,
                      lsw_mean_e_lower, ctx->acc.as<double>(), store, store_x, n_neighbour_bins);
}

int ansfm_lbl_accum_read(ansfm_ctx *ctx, double *out)
{
    CHECK_CTX(ctx);
    if (ctx->acc_nw <= 0) FAIL(ANSFM_ERR_INVALID, "lbl_accum_read: call ansfm_lbl_accum_begin first");
    if (!out) FAIL(ANSFM_ERR_INVALID, "lbl_accum_read: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(out, ctx->acc.p, (size_t)ctx->acc_L * ctx->acc_nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_lbl_accum_device_ptr(ansfm_ctx *ctx, double **dev, int *L, int *nw)
{
    CHECK_CTX(ctx);
    if (ctx->acc_nw <= 0) FAIL(ANSFM_ERR_INVALID, "lbl_accum_device_ptr: call ansfm_lbl_accum_begin first");
    if (!dev) FAIL(ANSFM_ERR_INVALID, "lbl_accum_device_ptr: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the caller may read the buffer from another stream
    *dev = ctx->acc.as<double>();
    if (L) *L = ctx->acc_L;
    if (nw) *nw = ctx->acc_nw;
    return ANSFM_OK;
}


/* ---- the line source resident in the context: runtime line-by-line as the opacity source of CIRSrad -------------------- */
} // extern "C"

// k rows of R distinct (gas, p, T, mix) rows into ctx->rt_k [R][H][nw] (H = 2: the (T + 5 K, p) spectrum behind every row):
// per gas, its rows are one batch of (T, p) points through the line and pseudo-continuum kernels, isotopologue by
// isotopologue -- lines_0, continuum_0, lines_1, ... onto one zeroed buffer (calc_klblg_online's order, LineData_0.py
// :2395-2459).  The points run in chunks whose constants fit ctx->rt_budget; a point's sums do not depend on its neighbours
// in a launch, so the chunk size changes no bit.  Rows are grouped by gas (checked by the callers); q_*: [R][isotopologues
// of the row's gas], one row after the other.
static int lblrt_compute(ansfm_ctx *ctx, int R, const int32_t *row_gas, const double *row_p, const double *row_t,
                         const double *row_mix, const double *q_lines, const double *q_cont, const double *q_lines_dT,
                         const double *q_cont_dT)
{
    const int S = ctx->rt_S, M = ctx->rt_M, nw = ctx->rt_nw, H = q_lines_dT ? 2 : 1;
    const size_t D = sizeof(double);
    HIPCHK(ctx->rt_k.reserve((size_t)R * H * nw * D));
    HIPCHK(hipMemsetAsync(ctx->rt_k.p, 0, (size_t)R * H * nw * D, ctx->stream));
    // the points of every gas, staged in one copy: per gas t, p [npt], mix [npt][M], then q_lines, q_cont [npt] per isotopologue
    std::vector<int> r0(S + 1, 0);
    for (int r = 0; r < R; ++r) r0[row_gas[r] + 1]++;
    for (int s = 0; s < S; ++s) r0[s + 1] += r0[s];
    std::vector<size_t> off(S + 1, 0);
    for (int s = 0; s < S; ++s) off[s + 1] = off[s] + (size_t)(r0[s + 1] - r0[s]) * H * (2 + M + 2 * ctx->rt_gas[s].size());
    std::vector<double> h(off[S]);
    size_t qbase = 0;
    for (int s = 0; s < S; ++s) {
        const int nr = r0[s + 1] - r0[s], npt = nr * H, niso = (int)ctx->rt_gas[s].size();
        double *t = h.data() + off[s], *p = t + npt, *mix = p + npt, *q = mix + (size_t)npt * M;
        for (int k = 0; k < npt; ++k) {
            const int r = r0[s] + k / H, hh = k % H;
            t[k] = hh ? row_t[r] + 5.0 : row_t[r];                                  // Spectroscopy_0.py:2021
            p[k] = row_p[r];
            for (int j = 0; j < M; ++j) mix[(size_t)k * M + j] = row_mix[(size_t)r * M + j];
            const size_t qo = qbase + (size_t)(k / H) * niso;
            for (int i = 0; i < niso; ++i) {
                q[(size_t)(2 * i) * npt + k] = hh ? q_lines_dT[qo + i] : q_lines[qo + i];
                q[(size_t)(2 * i + 1) * npt + k] = hh ? q_cont_dT[qo + i] : q_cont[qo + i];
            }
        }
        qbase += (size_t)nr * niso;
    }
    HIPCHK(ctx->rt_pts.reserve(h.size() * D + 8));
    HIPCHK(hipMemcpyAsync(ctx->rt_pts.p, h.data(), h.size() * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // h is a local buffer
    int chunks = 0;
    for (int s = 0; s < S; ++s) {
        const int nr = r0[s + 1] - r0[s], npt = nr * H, niso = (int)ctx->rt_gas[s].size();
        if (npt == 0) continue;
        const double *ht = h.data() + off[s], *hp = ht + npt, *hmix = hp + npt;
        const double *d_t = ctx->rt_pts.as<double>() + off[s], *d_p = d_t + npt, *d_mix = d_p + npt, *d_q = d_mix + (size_t)npt * M;
        size_t per_pt = 1;
        for (const auto &ip : ctx->rt_gas[s]) {
            per_pt = std::max(per_pt, (size_t)(kLblRows + 1) * ip->N);
            per_pt = std::max(per_pt, (size_t)(3 + (2 * ip->nb + 1) + 2) * ip->Nb);
        }
        const int C = (int)std::min<size_t>(std::min<size_t>((size_t)npt, 65535), std::max<size_t>(1, ctx->rt_budget / (per_pt * D)));
        HIPCHK(ctx->rt_scratch.reserve((size_t)C * per_pt * D));
        std::vector<double> mixmax(M, 0.0);
        for (int k = 0; k < npt; ++k)
            for (int j = 0; j < M; ++j) mixmax[j] = std::max(mixmax[j], fabs(hmix[(size_t)k * M + j]));
        for (int k0 = 0; k0 < npt; k0 += C, ++chunks) {
            const int Lc = std::min(C, npt - k0);
            double *d_out = ctx->rt_k.as<double>() + ((size_t)r0[s] * H + k0) * nw;
            for (int i = 0; i < niso; ++i) {
                const LblrtIso &iso = *ctx->rt_gas[s][i];
                if (iso.include_lines && iso.N > 0) {
                    // the shift of a line is at most sum_j |delta_j| mix_j |p / p_ref|; a wider bound only lengthens the line range
                    // that a block walks, and every line of it is tested against the windows again
                    double dmax = 0.0, pmax = 0.0;
                    for (int j = 0; j < M; ++j) dmax += iso.dabs[j] * mixmax[j];
                    for (int k = 0; k < npt; ++k) pmax = std::max(pmax, fabs(hp[k] / iso.p_ref));
                    const int N = iso.N;
                    const double *dl = iso.lines.as<double>();
                    LblParams p;
                    memset(&p, 0, sizeof p);
                    p.wn_grid = ctx->rt_grid.as<double>(); p.t_calc = d_t + k0; p.p_calc = d_p + k0; p.out = d_out;
                    p.q_ratio = d_q + (size_t)(2 * i) * npt + k0;
                    p.mmf = d_mix + (size_t)k0 * M; p.mmf_stride = M;
                    p.nu = dl; p.sw = dl + N; p.e_lower = dl + 2 * (size_t)N; p.stim_ref = dl + 3 * (size_t)N; p.bparams = dl + 4 * (size_t)N;
                    p.store = ctx->rt_scratch.as<double>();
                    p.shift = p.store + (size_t)Lc * kLblRows * N;
                    p.nw = nw; p.N = N; p.M = M; p.L = Lc; p.lineshape_id = iso.lineshape_id;
                    p.t_ref = iso.t_ref; p.p_ref = iso.p_ref; p.iso_abundance = iso.abundance; p.iso_mass = iso.mass; p.s_floor = iso.s_floor;
                    p.wn_calc_window = iso.wn_calc_window; p.wn_approx_window = iso.wn_approx_window;
                    p.max_shift = dmax * pmax * 1.0000001 + 1e-12;
                    hipLaunchKernelGGL(k_lbl_line_params, dim3(nblk((size_t)Lc * N, 256)), dim3(256), 0, ctx->stream, p);
                    hipLaunchKernelGGL(k_lbl_accumulate, dim3(nblk(nw, 256 * kLblPts), (unsigned)Lc), dim3(256), 0, ctx->stream, p);
                    HIPCHK(hipGetLastError());
                }
                if (iso.include_continuum && iso.Nb > 0) {
                    const int N = iso.Nb;
                    const size_t LN = (size_t)Lc * N;
                    const double *db = iso.bins.as<double>();
                    PcParams p;
                    memset(&p, 0, sizeof p);
                    p.centers = db; p.widths = db + N; p.sw = db + 2 * (size_t)N; p.e_lower = db + 3 * (size_t)N; p.lo = db + 4 * (size_t)N;
                    p.bparams = db + 5 * (size_t)N;
                    p.mmf = d_mix + (size_t)k0 * M; p.mmf_stride = M;
                    p.q_ratio = d_q + (size_t)(2 * i + 1) * npt + k0;
                    p.wn_grid = ctx->rt_grid.as<double>(); p.t_calc = d_t + k0; p.p_calc = d_p + k0; p.out = d_out;
                    p.store = ctx->rt_scratch.as<double>();
                    p.x = p.store + 3 * LN; p.ysum = p.x + LN; p.y = p.ysum + LN;
                    p.nw = nw; p.N = N; p.M = M; p.L = Lc; p.lineshape_id = iso.lineshape_id; p.nb = iso.nb;
                    p.first = iso.first; p.last = iso.last; p.jmax = iso.jmax;
                    p.t_ref = iso.t_cont; p.p_ref = iso.p_cont; p.iso_abundance = iso.abundance; p.iso_mass = iso.mass; p.wmax = iso.wmax;
                    hipLaunchKernelGGL(k_pc_params, dim3(nblk(LN, 256)), dim3(256), 0, ctx->stream, p);
                    hipLaunchKernelGGL(k_pc_shapes, dim3(nblk(LN, 256)), dim3(256), 0, ctx->stream, p);
                    hipLaunchKernelGGL(k_pc_gather, dim3(nblk(LN, 256)), dim3(256), 0, ctx->stream, p);
                    if (iso.jmax > 0)
                        hipLaunchKernelGGL(k_pc_interp, dim3(nblk((size_t)iso.jmax, 256), nblk((size_t)Lc, kPcLayers)), dim3(256), 0,
                                           ctx->stream, p);
                    HIPCHK(hipGetLastError());
                }
            }
        }
    }
    ctx->rt_last_rows = R; ctx->rt_last_points = R * H; ctx->rt_last_chunks = chunks;
    return ANSFM_OK;
}

extern "C" {

int ansfm_lblrt_begin(ansfm_ctx *ctx, int nw, const double *wn_grid, int S, int M)
{
    CHECK_CTX(ctx);
    ctx->rt_stage = 0; ctx->st_n = 0;
    if (ctx->lblrt) { ctx->lblrt = 0; ctx->have_table = false; }     // the committed source is taken apart
    if (nw <= 0 || S <= 0 || M <= 0 || !wn_grid) FAIL(ANSFM_ERR_INVALID, "lblrt_begin: bad argument");
    const int rc = lbl_grid_ascending(ctx, nw, wn_grid);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->rt_h_grid.assign(wn_grid, wn_grid + nw);
    HIPCHK(ctx->rt_grid.reserve((size_t)nw * sizeof(double)));
    HIPCHK(hipMemcpyAsync(ctx->rt_grid.p, ctx->rt_h_grid.data(), (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->rt_gas.clear();
    ctx->rt_gas.resize(S);
    ctx->rt_nw = nw; ctx->rt_S = S; ctx->rt_M = M; ctx->rt_stage = 1;
    return ANSFM_OK;
}

int ansfm_lblrt_add_isotopologue(ansfm_ctx *ctx, int gas, int lineshape_id, double isotopic_abundance, double isotopic_mass,
                                 int include_lines, int N, double t_ref, double p_ref, const double *broadening_params,
                                 const double *nu, const double *sw, const double *e_lower, const double *stim_ref, double s_floor,
                                 double wn_calc_window, double wn_approx_window, int include_continuum, int N_bins, double t_cont,
                                 double p_cont, const double *lsw_mean_broadening_params, const double *wn_bin_centers,
                                 const double *wn_bin_widths, const double *sw_sum, const double *lsw_mean_e_lower,
                                 int n_neighbour_bins)
{
    CHECK_CTX(ctx);
    if (ctx->rt_stage != 1) FAIL(ANSFM_ERR_INVALID, "lblrt_add_isotopologue: call ansfm_lblrt_begin first (and add before the commit)");
    if (gas < 0 || gas >= ctx->rt_S || N < 0 || N_bins < 0 || n_neighbour_bins < 0 ||
        (N > 0 && (!broadening_params || !nu || !sw || !e_lower || !stim_ref)) ||
        (N_bins > 0 && (!lsw_mean_broadening_params || !wn_bin_centers || !wn_bin_widths || !sw_sum || !lsw_mean_e_lower)))
        FAIL(ANSFM_ERR_INVALID, "lblrt_add_isotopologue: bad argument");
    if (n_neighbour_bins > kPcMaxNeighbours) FAIL(ANSFM_ERR_UNSUPPORTED, "pseudo-continuum: n_neighbour_bins 0 .. 8 are built");
    int rc = lbl_shape_built(ctx, lineshape_id);
    if (rc) return rc;
    const int M = ctx->rt_M;
    const size_t D = sizeof(double);
    std::unique_ptr<LblrtIso> iso(new LblrtIso());
    iso->lineshape_id = lineshape_id; iso->abundance = isotopic_abundance; iso->mass = isotopic_mass;
    iso->include_lines = include_lines ? 1 : 0; iso->include_continuum = include_continuum ? 1 : 0;
    iso->t_ref = t_ref; iso->p_ref = p_ref; iso->s_floor = s_floor; iso->wn_calc_window = wn_calc_window;
    iso->wn_approx_window = wn_approx_window; iso->t_cont = t_cont; iso->p_cont = p_cont; iso->nb = n_neighbour_bins;
    iso->dabs.assign(M, 0.0);
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<double> h, hb;
    if (N > 0) {     // no lines: LineSetSpecData.has_data == False, nothing is added (LineData_0.py:845)
        std::vector<int> ord;
        lbl_pack_lines(M, N, broadening_params, nu, sw, e_lower, stim_ref, ord, h);
        for (int j = 0; j < M; ++j)
            for (int i = 0; i < N; ++i) iso->dabs[j] = std::max(iso->dabs[j], fabs(broadening_params[(size_t)(3 * j + 2) * N + i]));
        HIPCHK(iso->lines.reserve(h.size() * D));
        HIPCHK(hipMemcpyAsync(iso->lines.p, h.data(), h.size() * D, hipMemcpyHostToDevice, ctx->stream));
        iso->N = N;
    }
    bool any = false;
    for (int i = 0; i < N_bins; ++i) any = any || sw_sum[i] != 0;
    if (any) {       // all sums zero: PseudoContSpecData.has_data == False (:1244, :1336)
        PcGeometry g;
        if ((rc = lbl_pc_geometry(ctx, ctx->rt_nw, ctx->rt_h_grid.data(), N_bins, wn_bin_centers, wn_bin_widths, g))) return rc;
        const size_t n = N_bins;
        hb.resize((5 + 3 * (size_t)M) * n);
        for (size_t i = 0; i < n; ++i) {
            hb[i] = wn_bin_centers[i]; hb[n + i] = wn_bin_widths[i]; hb[2 * n + i] = sw_sum[i]; hb[3 * n + i] = lsw_mean_e_lower[i];
            hb[4 * n + i] = g.lo[i];
        }
        memcpy(hb.data() + 5 * n, lsw_mean_broadening_params, 3 * (size_t)M * n * D);
        HIPCHK(iso->bins.reserve(hb.size() * D));
        HIPCHK(hipMemcpyAsync(iso->bins.p, hb.data(), hb.size() * D, hipMemcpyHostToDevice, ctx->stream));
        iso->Nb = N_bins; iso->first = g.first; iso->last = g.last; iso->jmax = g.jmax; iso->wmax = g.wmax;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));   // h / hb are local buffers
    ctx->rt_gas[gas].push_back(std::move(iso));
    return ANSFM_OK;
}

int ansfm_lblrt_commit(ansfm_ctx *ctx)
{
    CHECK_CTX(ctx);
    if (ctx->rt_stage < 1) FAIL(ANSFM_ERR_INVALID, "lblrt_commit: call ansfm_lblrt_begin first");
    for (const auto &g : ctx->rt_gas)
        if (g.empty()) FAIL(ANSFM_ERR_INVALID, "lblrt_commit: every gas needs at least one isotopologue (ansfm_lblrt_add_isotopologue)");
    HIPCHK(hipSetDevice(ctx->device));
    // the context answers like an LBL table with G = 1 and W = nw: the table's bookkeeping (wave grid, the single
    // g-ordinate, paddings) comes from the table uploader on a 2 x 2 table of zeros that no kernel reads in this mode
    const int W = ctx->rt_nw, S = ctx->rt_S;
    const size_t n = (size_t)W * 4 * S;
    HIPCHK(ctx->tmp_in.reserve(n * sizeof(double)));
    HIPCHK(hipMemsetAsync(ctx->tmp_in.p, 0, n * sizeof(double), ctx->stream));
    const double pt[2] = {1.0, 2.0}, one = 1.0;
    const int rc = ansfm_upload_ktable_dev(ctx, W, 1, 2, 2, S, ctx->tmp_in.as<double>(), pt, pt, ctx->rt_h_grid.data(), &one);
    ctx->tmp_in.release();
    if (rc) return rc;
    ctx->is_lbl = 1; ctx->temp2d = 0; ctx->monotone = 1;
    ctx->lblrt = 1; ctx->rt_stage = 2; ctx->st_n = 0;
    return ANSFM_OK;
}

int ansfm_lblrt_set_scratch_bytes(ansfm_ctx *ctx, int64_t bytes)
{
    CHECK_CTX(ctx);
    if (bytes <= 0) FAIL(ANSFM_ERR_INVALID, "lblrt_set_scratch_bytes: bad argument");
    ctx->rt_budget = (size_t)bytes;
    return ANSFM_OK;
}

int ansfm_lblrt_last(const ansfm_ctx *ctx, int *rows, int *points, int *chunks)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (rows) *rows = ctx->rt_last_rows;
    if (points) *points = ctx->rt_last_points;
    if (chunks) *chunks = ctx->rt_last_chunks;
    return ANSFM_OK;
}

int ansfm_lblrt_set_state(ansfm_ctx *ctx, int n_models, int L, int R, const int32_t *krow, const int32_t *row_gas,
                          const double *row_p_atm, const double *row_t, const double *row_mix, const double *row_q_lines,
                          const double *row_q_cont, const double *row_q_lines_dT, const double *row_q_cont_dT)
{
    CHECK_CTX(ctx);
    ctx->st_n = 0;
    if (!ctx->lblrt) FAIL(ANSFM_ERR_INVALID, "lblrt_set_state: commit a line source first (ansfm_lblrt_commit)");
    if (n_models <= 0 || L <= 0 || R <= 0 || !krow || !row_gas || !row_p_atm || !row_t || !row_mix || !row_q_lines || !row_q_cont ||
        (row_q_lines_dT == nullptr) != (row_q_cont_dT == nullptr))
        FAIL(ANSFM_ERR_INVALID, "lblrt_set_state: bad argument");
    const int S = ctx->rt_S;
    // the maps, before anything is launched
    for (int r = 0; r < R; ++r)
        if (row_gas[r] < 0 || row_gas[r] >= S || (r > 0 && row_gas[r] < row_gas[r - 1]))
            FAIL(ANSFM_ERR_INVALID, "lblrt_set_state: row_gas[" + std::to_string(r) + "] = " + std::to_string(row_gas[r]) +
                                        " is outside [0, S = " + std::to_string(S) + ") or below its predecessor (rows are grouped by gas)");
    const size_t nk = (size_t)n_models * S * L;
    for (size_t i = 0; i < nk; ++i) {
        const int s = (int)((i / L) % S);
        if (krow[i] < 0 || krow[i] >= R || row_gas[krow[i]] != s)
            FAIL(ANSFM_ERR_INVALID, "lblrt_set_state: krow[" + std::to_string(i / ((size_t)S * L)) + "][" + std::to_string(s) + "][" +
                                        std::to_string(i % L) + "] = " + std::to_string(krow[i]) + " is outside [0, R = " + std::to_string(R) +
                                        ") or a row of another gas");
    }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ctx->rt_krow.reserve(nk * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(ctx->rt_krow.p, krow, nk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const int rc = lblrt_compute(ctx, R, row_gas, row_p_atm, row_t, row_mix, row_q_lines, row_q_cont, row_q_lines_dT, row_q_cont_dT);
    if (rc) return rc;           // (lblrt_compute synchronises after its staging copy: krow is the caller's)
    ctx->st_n = n_models; ctx->st_L = L; ctx->st_R = R; ctx->st_H = row_q_lines_dT ? 2 : 1;
    return ANSFM_OK;
}

static int calc_klbl_online_impl(ansfm_ctx *ctx, const char *fn, int L, const double *press, const double *temp,
                                 const double *mol_mix_frac, const double *q_lines, const double *q_cont,
                                 const double *q_lines_dT, const double *q_cont_dT, double *k_out, double *dkdT_out)
{
    CHECK_CTX(ctx);
    if (!ctx->lblrt) { ctx->err = std::string(fn) + ": commit a line source first (ansfm_lblrt_commit)"; return ANSFM_ERR_NOTABLE; }
    if (L <= 0 || !press || !temp || !mol_mix_frac || !q_lines || !q_cont || !k_out || (dkdT_out && (!q_lines_dT || !q_cont_dT))) {
        ctx->err = std::string(fn) + ": bad argument";
        return ANSFM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(ctx->device));
    ctx->st_n = 0;                                  // the rows of a pending state are overwritten
    const int S = ctx->rt_S, M = ctx->rt_M, W = ctx->rt_nw, R = S * L;
    size_t niso_all = 0;
    for (const auto &g : ctx->rt_gas) niso_all += g.size();
    std::vector<int32_t> row_gas(R);
    std::vector<double> rp(R), rt(R), rmix((size_t)R * M), q[4];
    const double *qsrc[4] = {q_lines, q_cont, dkdT_out ? q_lines_dT : nullptr, dkdT_out ? q_cont_dT : nullptr};
    for (int a = 0; a < 4; ++a) if (qsrc[a]) q[a].resize(niso_all * L);
    size_t qo = 0, ib = 0;
    for (int s = 0; s < S; ++s) {
        const size_t niso = ctx->rt_gas[s].size();
        for (int l = 0; l < L; ++l) {
            const int r = s * L + l;
            row_gas[r] = s; rp[r] = press[l]; rt[r] = temp[l];
            for (int j = 0; j < M; ++j) rmix[(size_t)r * M + j] = mol_mix_frac[(size_t)s * M + j];
            for (size_t i = 0; i < niso; ++i, ++qo)
                for (int a = 0; a < 4; ++a) if (qsrc[a]) q[a][qo] = qsrc[a][(ib + i) * L + l];
        }
        ib += niso;
    }
    int rc = lblrt_compute(ctx, R, row_gas.data(), rp.data(), rt.data(), rmix.data(), q[0].data(), q[1].data(),
                           qsrc[2] ? q[2].data() : nullptr, qsrc[3] ? q[3].data() : nullptr);
    if (rc) return rc;
    const size_t n = (size_t)W * L * S;
    HIPCHK(ctx->tmp_out.reserve(n * sizeof(double) * (dkdT_out ? 2 : 1)));
    double *dk = dkdT_out ? ctx->tmp_out.as<double>() + n : nullptr;
    hipLaunchKernelGGL(k_lblrt_seam, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, ctx->rt_k.as<double>(), dkdT_out ? 2 : 1, W, S, L,
                       ctx->tmp_out.as<double>(), dk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(k_out, ctx->tmp_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (dkdT_out) HIPCHK(hipMemcpyAsync(dkdT_out, dk, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_calc_klbl_online(ansfm_ctx *ctx, int L, const double *press, const double *temp, const double *mol_mix_frac,
                           const double *q_lines, const double *q_cont, double *k_out)
{
    return calc_klbl_online_impl(ctx, "calc_klbl_online", L, press, temp, mol_mix_frac, q_lines, q_cont, nullptr, nullptr, k_out,
                                 nullptr);
}

int ansfm_calc_klblg_online(ansfm_ctx *ctx, int L, const double *press, const double *temp, const double *mol_mix_frac,
                            const double *q_lines, const double *q_cont, const double *q_lines_dT, const double *q_cont_dT,
                            double *k_out, double *dkdT_out)
{
    if (ctx && !dkdT_out) { ctx->err = "calc_klblg_online: bad argument"; return ANSFM_ERR_INVALID; }
    return calc_klbl_online_impl(ctx, "calc_klblg_online", L, press, temp, mol_mix_frac, q_lines, q_cont, q_lines_dT, q_cont_dT,
                                 k_out, dkdT_out);
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

/* ---- Mie theory over a particle size distribution (Scatter_0.makephase) ---------------------------------------------------- */
namespace {
constexpr int kMieBlockDefault = 512;                  // radii per block
constexpr int kMieCapDefault = 1 << 20;                // radii of an open range before "did not terminate"
constexpr size_t kMieWorkspaceMax = (size_t)1 << 30;   // bytes of D_n and coefficients one block may take
}

extern "C" {

int ansfm_mie_set_radius_block(ansfm_ctx *ctx, int radii)
{
    CHECK_CTX(ctx);
    if (radii < 0 || radii % kMieChunk) FAIL(ANSFM_ERR_INVALID, "mie_set_radius_block: the block is a multiple of 64 radii (0 = default)");
    ctx->mie_block = radii;
    return ANSFM_OK;
}

int ansfm_mie_set_radius_cap(ansfm_ctx *ctx, int radii)
{
    CHECK_CTX(ctx);
    if (radii < 0) FAIL(ANSFM_ERR_INVALID, "mie_set_radius_cap: the cap is a number of radii (0 = default)");
    ctx->mie_cap = radii;
    return ANSFM_OK;
}

int ansfm_mie_last(const ansfm_ctx *ctx, double *kernel_ms, int32_t *blocks, int32_t *block_radii)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (kernel_ms) *kernel_ms = ctx->mie_ms;
    if (blocks) *blocks = ctx->mie_blocks;
    if (block_radii) *block_radii = ctx->mie_block_radii;
    return ANSFM_OK;
}

int ansfm_mie_makephase(ansfm_ctx *ctx, int nwave, const double *wavel_um, int iscat, const double dsize[3], const double rs[3],
                        const double *refindx, int ntheta, const double *theta_deg, double *xscat, double *xext, double *phas,
                        int32_t *n_radii)
{
    CHECK_CTX(ctx);
    char msg[256];
    if (nwave <= 0 || nwave > 65535 || ntheta <= 0 || ntheta > 4096 || !wavel_um || !dsize || !rs || !refindx || !theta_deg ||
        !xscat || !xext || !phas)
        FAIL(ANSFM_ERR_INVALID, "mie_makephase: bad argument");
    if (iscat < 1 || iscat > 4) {
        snprintf(msg, sizeof msg, "mie_makephase: iscat %d is not a Mie case (1 .. 4)", iscat);
        FAIL(ANSFM_ERR_INVALID, msg);
    }
    int n90 = 0;
    std::vector<double> h_in((size_t)3 * nwave + 2 * ntheta);
    double *h_wavel = h_in.data(), *h_ref = h_wavel + nwave, *h_cs = h_ref + 2 * nwave, *h_s2 = h_cs + ntheta;
    for (int j = 0; j < ntheta; ++j) {
        const double th = theta_deg[j];
        if (!(th >= 0.0 && th <= 90.0)) {
            snprintf(msg, sizeof msg, "mie_makephase: scattering angle %g (index %d) is outside [0, 90]", th, j);
            FAIL(ANSFM_ERR_INVALID, msg);
        }
        n90 += th == 90.0;
        // dmie :1472-1485
        if (th == 0.0) { h_cs[j] = 1.0; h_s2[j] = 0.0; }
        else if (th == 90.0) { h_cs[j] = 0.0; h_s2[j] = 1.0; }
        else { h_cs[j] = std::cos(M_PI * th / 180.0); h_s2[j] = 1.0 - h_cs[j] * h_cs[j]; }
    }
    const int nphas = n90 == 1 ? 2 * ntheta - 1 : 2 * ntheta;
    for (int w = 0; w < nwave; ++w) {
        if (!(wavel_um[w] > 0.0) || !std::isfinite(wavel_um[w]) || !std::isfinite(refindx[2 * w]) || !std::isfinite(refindx[2 * w + 1])) {
            snprintf(msg, sizeof msg, "mie_makephase: wavelength %g um (index %d) or its refractive index is not usable", wavel_um[w], w);
            FAIL(ANSFM_ERR_INVALID, msg);
        }
        h_wavel[w] = wavel_um[w]; h_ref[2 * w] = refindx[2 * w]; h_ref[2 * w + 1] = refindx[2 * w + 1];
    }
    if (!(rs[0] > 0.0) || !(rs[2] > 0.0) || !std::isfinite(rs[0]) || !std::isfinite(rs[1]) || !std::isfinite(rs[2]))
        FAIL(ANSFM_ERR_INVALID, "mie_makephase: the first radius rs[0] and the step rs[2] must be positive");
    const int cap = ctx->mie_cap ? ctx->mie_cap : kMieCapDefault;
    const int B = ctx->mie_block ? ctx->mie_block : kMieBlockDefault;

    MieParams p{};
    p.nwave = nwave; p.ntheta = ntheta; p.nphas = nphas; p.iscat = iscat;
    p.d0 = dsize[0]; p.d1 = dsize[1]; p.d2 = dsize[2];
    p.r1 = rs[0]; p.delr = rs[2]; p.sqrt2pi = std::sqrt(2.0 * M_PI);
    if (rs[1] < rs[0]) {              // open range: ends where n Q_sca has fallen to 1e-6 of its maximum beyond r_peak (:1693-1709)
        p.inr = 0; p.mend = cap; p.rmax = 0.0;
        if (dsize[1] != 0.0) {
            if (iscat == 1) p.rmax = dsize[2] * dsize[0] * dsize[1];
            else if (iscat == 2) p.rmax = std::exp(std::log(dsize[0]) - dsize[1] * dsize[1]);
            else if (iscat == 3) p.rmax = std::pow(dsize[0] / (dsize[1] * dsize[2]), 1.0 / dsize[2]);
        }
    } else {                          // closed range (:1683-1685)
        const double q = (rs[1] - rs[0]) / rs[2];
        if (!(q < (double)cap)) {
            snprintf(msg, sizeof msg, "mie_makephase: a closed range of %g radii is above the cap of %d", q + 1.0, cap);
            FAIL(ANSFM_ERR_INVALID, msg);
        }
        int inr = 1 + (int)q;
        if (inr > 1 && inr % 2 != 0) ++inr;
        p.inr = inr; p.mend = inr;
    }

    HIPCHK(hipSetDevice(ctx->device));
    const size_t T = (size_t)nwave * B, D = sizeof(double), NT = (size_t)nwave * (ntheta + 1) * 3;
    if (T > ((size_t)1 << 26)) FAIL(ANSFM_ERR_INVALID, "mie_makephase: wavelengths times the radius block exceed 2^26; set a smaller block");
    // doubles: inputs | qext qsca anr [T] | nqmax [nwave] | partial | total | xscat xext [nwave] phas; then the int arrays
    const size_t n_in = h_in.size(), n_part = (size_t)(B / kMieChunk) * NT;
    const size_t n_dbl = n_in + 3 * T + nwave + n_part + NT + 2 * (size_t)nwave + (size_t)nwave * nphas;
    HIPCHK(ctx->mie_st.reserve(n_dbl * D + (2 * T + 3 * (size_t)nwave) * sizeof(int)));
    double *d = ctx->mie_st.as<double>();
    p.wavel = d; p.refindx = d + nwave; p.cstht = d + 3 * (size_t)nwave; p.si2tht = p.cstht + ntheta; d += n_in;
    p.qext = d; p.qsca = d + T; p.anr = d + 2 * T; d += 3 * T;
    p.nqmax = d; d += nwave;
    p.partial = d; d += n_part;
    p.total = d; d += NT;
    p.xscat = d; p.xext = d + nwave; p.phas = d + 2 * (size_t)nwave; d += 2 * (size_t)nwave + (size_t)nwave * nphas;
    int *di = reinterpret_cast<int *>(d);
    p.nterm = di; p.fail = di + T; p.mcut = di + 2 * T; p.failcode = p.mcut + nwave; p.failm = p.failcode + nwave;
    std::vector<int> h_state((size_t)3 * nwave, 0);
    std::fill(h_state.begin(), h_state.begin() + nwave, INT_MAX);
    HIPCHK(hipMemcpyAsync(const_cast<double *>(p.wavel), h_in.data(), n_in * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(p.mcut, h_state.data(), h_state.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(p.nqmax, 0, (size_t)nwave * D, ctx->stream));
    HIPCHK(hipMemsetAsync(p.total, 0, NT * D, ctx->stream));

    ctx->mie_ms = 0; ctx->mie_blocks = 0; ctx->mie_block_radii = 0;
    // the largest |m| / lambda bounds nmx2 of a block from its last radius
    double mk = 0.0;
    for (int w = 0; w < nwave; ++w)
        mk = std::max(mk, std::sqrt(h_ref[2 * w] * h_ref[2 * w] + h_ref[2 * w + 1] * h_ref[2 * w + 1]) / h_wavel[w]);
    int m0 = 0;
    for (;;) {
        if (m0 >= p.mend) {
            if (p.inr) break;
            snprintf(msg, sizeof msg, "mie_makephase: size integration did not terminate within %d radii", cap);
            FAIL(ANSFM_ERR_INVALID, msg);
        }
        int nrad = B;
        size_t ws = 0;
        int NH = 0;
        for (;;) {
            const int mlast = std::min(m0 + nrad, p.mend) - 1;
            const double t0 = 2.0 * M_PI * (p.r1 + (double)mlast * p.delr) * mk * (1.0 + 1e-9);
            NH = 1.1 * t0 > 150.0 ? (int)std::min(t0, (double)kMieNcap / 1.1) + 2 : 136;   // a radius that gives up at nmx1 stores nothing
            ws = (size_t)NH * 6 * nwave * nrad * D;
            if (ws <= kMieWorkspaceMax || nrad == kMieChunk) break;
            nrad = std::max(kMieChunk, nrad / 2 / kMieChunk * kMieChunk);
        }
        if (ws > kMieWorkspaceMax) FAIL(ANSFM_ERR_UNSUPPORTED, "mie_makephase: size parameters whose series do not fit the workspace");
        HIPCHK(ctx->mie_ws.reserve(ws));
        const size_t Tb = (size_t)nwave * nrad;
        p.m0 = m0; p.nrad = nrad; p.NH = NH;
        p.acap = ctx->mie_ws.as<double>(); p.coef = p.acap + (size_t)NH * 2 * Tb;
        HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
        hipLaunchKernelGGL(k_mie_coeff, dim3(nblk(Tb, 256)), dim3(256), 0, ctx->stream, p);
        hipLaunchKernelGGL(k_mie_cutoff, dim3(nblk(nwave, 64)), dim3(64), 0, ctx->stream, p);
        hipLaunchKernelGGL(k_mie_angles, dim3(nrad / kMieChunk, nwave, nblk(ntheta + 1, kMieAngleWaves)),
                           dim3(kMieChunk * kMieAngleWaves), 0, ctx->stream, p);
        hipLaunchKernelGGL(k_mie_accum, dim3(nblk(NT, 256)), dim3(256), 0, ctx->stream, p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
        HIPCHK(hipMemcpyAsync(h_state.data(), p.mcut, h_state.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        ctx->mie_ms += ms; ctx->mie_blocks += 1; ctx->mie_block_radii = std::max(ctx->mie_block_radii, nrad);
        bool all = true;
        for (int w = 0; w < nwave; ++w) {
            const int code = h_state[nwave + w], m = h_state[2 * (size_t)nwave + w];
            if (code) {
                const char *why = code == 1 ? "the logarithmic derivative would start at order 29999 or above"
                                  : code == 2 ? "the series needs more than nmx2 = max(135, int(|m| x)) terms" : "workspace too small";
                snprintf(msg, sizeof msg, "mie_makephase: wavelength %g um (index %d), radius %g um (index %d): %s", h_wavel[w], w,
                         p.r1 + (double)m * p.delr, m, why);
                FAIL(ANSFM_ERR_INVALID, msg);
            }
            all = all && h_state[w] != INT_MAX;
        }
        if (all) break;
        m0 += nrad;
    }
    hipLaunchKernelGGL(k_mie_finish, dim3(nblk((size_t)nwave * nphas, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(xscat, p.xscat, (size_t)nwave * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(xext, p.xext, (size_t)nwave * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(phas, p.phas, (size_t)nwave * nphas * D, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (n_radii)
        for (int w = 0; w < nwave; ++w) n_radii[w] = h_state[w] + 1;
    return ANSFM_OK;
}

}  // extern "C"
