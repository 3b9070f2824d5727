// ansfm_ctx.hip.h -- what the host translation units of libansfm.so share: the context, the error macros, the staging of
// host pointers and the declarations of the host helpers that one unit defines and another calls.  No kernel lives here, and
// no kernel header is included: a header that defines kernels belongs to exactly one .hip.
//   ansfm_api.hip      lifecycle, tables, the gas-opacity stage, the entry points of thermal / transmission / single-scattering
//                      RT and its gradients (their arguments travel as one record, RtCall)
//   ansfm_overlap.hip  forward merge of the correlated-k path (64-bit keys); ansfm_merge32.hip: the 32-bit-key merge;
//                      what a call launches is planned in ansfm_merge_plan.h (host only, no HIP header)
//   ansfm_overlapg.hip gradient merge
//   ansfm_rt.hip       thermal / transmission / single-scattering RT kernels and their gradients
//   ansfm_scatter.hip  multiple scattering
//   ansfm_lbl.hip      runtime line-by-line
//   ansfm_ops.hip      gradient maps, ILS convolution, continua, layering, the k-distribution entry
//   ansfm_mie.hip      Mie theory over size distributions
//   ansfm_hgfit.hip    double Henyey-Greenstein fit of phase functions
//   ansfm_phase.hip    aerosol phase functions on the calculation grid (calc_phase, calc_phase_ray) and their resident source
//   ansfm_surface.hip  surface reflection: the BRDF at points and the BRDF matrix
//   ansfm_transit.hip, ansfm_occultation.hip, ansfm_limb.hip, ansfm_disc.hip  the fused gradient routes, collapsed over the
//                      paths (transit), with the tangent paths mixed to the geometries (occultation, limb) or with the averaging
//                      points of a disc mixed to the geometries (disc) on the device: each its entry point,
//                      its index and matrix build, its scratch layout and its launcher.  What they share is in
//                      ansfm_pathmix.hip.h (host: checks, path matrix, prologue, staged call, *_last) and
//                      ansfm_pathmix_kernels.hip.h (device functions: path pass, contraction, sums over g)
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <memory>
#include <string>
#include <map>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/ansfm.h"
#pragma GCC visibility pop
#include "ansfm_merge_plan.h"
#include "ansfm_ms_variants.h"

namespace ansfm {

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

// What a fused gradient route (transit, occultation, limb, disc) keeps between calls: its scratch beyond the gas stage, the bytes of
// it the last call needed, whether a call is recorded, and the events around its two kernel stages (created at the first call)
struct FusedRoute {
    DevBuf ws;
    size_t scratch_bytes = 0;
    int recorded = 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double ms[2] = {0.0, 0.0};   // disc: the times between the events, read once when the call ends (the others query in *_last)
};

}  // namespace ansfm

using ansfm::DevBuf;
using ansfm::FusedRoute;
using ansfm::LblrtIso;

// ints of ansfm_ctx::d_flag: 0 the upload kernels' flag, 1 "unsorted input", 12 the de-duplication's row counter, 13 the
// merge redo count; from kFlagTileCounter the merge kernels' eight tile queues and, behind them, the forward merge's five
// 64-bit totals (row-major merges, all merges, non-zero pattern bytes read, rows walked behind a list phase, merges walked on
// the static schedule), which one memset per launch clears together
// (merge_launch_begin)
constexpr int kFlagInts = 40, kFlagTileCounter = 16, kMergeTotals = 5;
static_assert(kFlagTileCounter + 8 + 2 * kMergeTotals <= kFlagInts, "the totals lie inside d_flag");

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
    std::map<const void *, size_t> merge_lds_allowed;   // dynamic LDS each merge kernel has been allowed on this device
    ansfm::MergePlan last_merge;    // the last forward merge launch (ansfm_last_merge_launch, _group_width, _table_layout)
    int merge_keys = 64;     // 32: run the forward merge on k_ck_overlap32's float32 keys (ansfm_set_merge_keys)
    // The wavenumber order of the forward merge (MergePlan::order): two buffers of Wpad pattern bytes, merge_hint [2][Wpad].  A
    // launch reads buffer merge_hint_parity and writes the other, and the parity flips after it.  The bytes are valid for the
    // next launch while its key equals the writer's: the source (table_generation, 0 for the seam), W, Wpad, the rows
    // n_models * L, S and G; any other qualifying launch clears both buffers first and so runs in the identity order.
    DevBuf merge_hint;
    int merge_hint_parity = 0;
    struct MergeHintKey {
        long source = -1;
        int W = 0, Wpad = 0, R = 0, S = 0, G = 0;
        bool operator==(const MergeHintKey &o) const
        {
            return source == o.source && W == o.W && Wpad == o.Wpad && R == o.R && S == o.S && G == o.G;
        }
    } merge_hint_key;               // source < 0: no launch has written a hint
    long table_generation = 0;      // counts the uploads of a table (ansfm_upload_ktable*)
    int last_merge_G = 0;              // the g-ordinates of the last forward merge launch (ansfm_last_merge_suffix)
    bool last_merge_ordered = false;   // the last forward merge launch read valid pattern bytes (ansfm_last_merge_order)
    bool have_table = false;
    int grid_f32 = 0, delg_f32 = 0;
    int is_lbl = 0, temp2d = 0;   // LBL-table mode (ILBL=2): G = 1, TEMP may be [NP][NT]
    DevBuf lnK, d_press, d_temp, d_wave, d_delg, d_flag;
    // the g-fastest copy of lnK, [NP][NT][S][Wpad][Gs] (build_table_gfast, ansfm_ktable_gfast): lnKg_bytes is its size for the
    // table in lnK, 0 when that table has none (G = 1, an LBL table, ANSFM_TABLE_GFAST=0, a failed allocation)
    DevBuf lnKg;
    size_t lnKg_bytes = 0;
    std::vector<double> h_delg;
    // resident continuum sources on the table's grid (ansfm_upload_cia / ansfm_upload_dust; a new table clears them)
    //   cia_tab: cia_waven [NWC], K_CIA [NPAIR][NPE][NT][NWC], cia_temp [NT], cia_frac [nfrac], k_co2, k_n2n2, k_n2h2 [W] each
    //   cia_idx: igas1, igas2 [NPAIR];  cia_lay: the CiaLayer records of a call's rows;  dust_kext: kext_w [NDUST][Wpad];
    //   dust_ksca: ksca_w [NDUST][Wpad], the scattering cross sections beside it (the multiple-scattering continuum reads them)
    DevBuf cia_tab, cia_idx, cia_lay, dust_kext, dust_ksca;
    int cia_on = 0, cia_ispace = 0, cia_NWC = 0, cia_NPAIR = 0, cia_NPE = 0, cia_NT = 0, cia_nfrac = 0, cia_NPARA = 0, cia_NVMR = 0,
        cia_ico2 = -1, cia_in2 = -1, cia_ih2 = -1, cia_covers = 0;
    int dust_n = 0;                         // NDUST of the uploaded aerosol source, 0: none

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
    DevBuf ms_cont_rows;                 // ansfm_cirsrad_ck_scatter_batch_cont: the rows k_ms_cont_rows forms, TAUCIA / TAUDUST / TAURAY / TAUSCAT [R][W] and the fractions [R][ncont][W]
    DevBuf ms_phas_src;                  // ansfm_cirsrad_ck_scatter_batch_src: phasarr [ncont][W][2][nth] formed from the phase-function source
    DevBuf ss_cont_rows, ss_phase_fn;    // ansfm_cirsrad_ck_singlescatt_batch_cont: the rows k_ss_cont_rows forms, sca [R][Wpad] and phase [P][R][Wpad]; phase_fn [W][P][ncont + 1]
    DevBuf ms_tauray_l, ms_lfrac_l;      // the continuum by rows: TAURAY / aerosol fractions of a launch's models (the model-by-model route: one model's dense arrays)
    DevBuf ms_cache, ms_orders, ms_same, ms_pcache, ms_lstart; // batched scattering Jacobian: doubled layers / prefix stacks of model 0, orders cached, layer flags, sweep starts
    long ms_cache_hits = 0, ms_cache_layers = 0;   // (model, layer) pairs taken from the cache / all, last batch call
    // per-model phase functions of the batch (ansfm_set_phase_variants): the pending setting (host copies, consumed by the next
    // batched scattering call), the variants' phasarr [V - 1][ncont][W][2][nth] and the small tables (pairs, the models' variants,
    // the differing components) on the device; (variant, component) pairs integrated and walked / bytes of the variants' phase
    // matrices and factors in the last batched call (ansfm_last_scatter_variants)
    ansfm::MsVariantSet ms_pv;
    DevBuf ms_var_in, ms_var_tab;
    long ms_var_pairs = 0, ms_var_bytes = 0;
    hipEvent_t ms_walk_ev[2] = {nullptr, nullptr};   // around the phase matrices and the walk of the last batched call at G > 1
    bool ms_walk_timed = false;
    long ms_windows = 0, ms_window_w = 0;          // spectral windows of phase matrices / Hansen factors of the last scattering call, their size
    DevBuf hb[25];  // staging buffers of the host-pointer entry points
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
    // double Henyey-Greenstein fit (ansfm_hg_fit): cos(theta), the phase functions, the results and the per-fit counts and
    // flags; kernel time of the last call
    DevBuf hg_st;
    double hg_ms = 0;
    // aerosol phase functions.  phase_src: the resident source on the table's grid (ansfm_upload_phase; a new table clears it) --
    //   Scatter.WAVE [NWS], Scatter.THETA [NTAB] (IMIE 1), the tables, x_lo / x_hi [W] of every wavenumber's interval, f_w / g1_w /
    //   g2_w [3][NDUST][Wpad] (IMIE 0), lo [W] (int32); phase_h_theta: Scatter.THETA on the host, for the angle check.
    // phase_ws: the angles of a launch from the source (theta, mu, cos theta, brackets); phase_call: the staged inputs and the
    //   result of an array-level call; kernel time of the last such call
    DevBuf phase_src, phase_ws, phase_call;
    int phase_n = 0;                        // NDUST of the uploaded phase-function source, 0: none
    int phase_imie = 0, phase_NWS = 0, phase_NTAB = 0;
    std::vector<double> phase_h_theta;
    double phase_ms = 0;
    // surface reflection (ansfm_surface_brdf, ansfm_brdf_matrix): the result, the per-azimuth table, kernel time of the last call
    DevBuf brdf_out, brdf_azi;
    double brdf_ms = 0;
    // the fused gradient routes; ws holds
    //   transit (ansfm_cirsradg_ck_transit): A [L][G][Wpad] + exp(-tau_path) [P][G][Wpad] + AREA [W] + T [W][P]
    //   occ (ansfm_cirsradg_ck_occultation): exp(-tau_path) [P][G][Wpad] + MOD [W][Q] + T [W][P]
    //   limb (ansfm_cirsradg_ck_limb): the Planck tables [2][NT][Wpad] + spec [P][G][Wpad] + dg E [Q][L][G][Wpad] + the partial
    //   sums of Z [GS][Q][L][Wpad] + MOD [W][Q] + SPEC [W][P]
    //   disc (ansfm_cirsradg_ck_disc): the Planck tables [2][NT + 1][Wpad] + spec [P][G][Wpad] + dg E [Q][L][G][Wpad] + the
    //   partial sums of Z [GS][Q][L][Wpad] + the ground's sums [Q][G][Wpad] + MOD, dTSMOD [W][Q] + SPEC [W][P]
    FusedRoute transit, occ, limb, disc;

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
        for (FusedRoute *r : {&transit, &occ, &limb, &disc})
            for (hipEvent_t e : r->ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ms_ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ms_walk_ev) if (e) (void)hipEventDestroy(e);
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

namespace ansfm {

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
static inline unsigned nblk(size_t n, int b) { return (unsigned)((n + b - 1) / b); }

/* ---- helpers that one translation unit defines and another calls ------------------------------------------------------- */
// ansfm_api.hip, the gas-opacity stage (described where they are defined)
int gas_tau(ansfm_ctx *ctx, int n, int L, const double *press, const double *temp, const double *amount, bool generic,
            double *dk = nullptr);
int gas_opacity(ansfm_ctx *ctx, int rows, const double *press, const double *temp, const double *amount);
struct DedupRows {
    int rows;
    const double *press, *temp, *amount;
};
// further per-layer inputs that are part of a row's identity: arrays [n L][width] (ansfm_table_kernels.hip.h)
struct DedupCols;
int dedup_rows(ansfm_ctx *ctx, int n, int L, const double *press, const double *temp, const double *amount,
               const DedupCols *cols, DedupRows *out);
// a table has been uploaded: the continuum sources on the old grid go (dust_n = 0: kext_w and ksca_w alike), and the
// phase-function source with them
inline void clear_continuum_sources(ansfm_ctx *ctx) { ctx->cia_on = 0; ctx->dust_n = 0; ctx->phase_n = 0; }
// A continuum formed from the context's resident sources (ansfm_upload_cia, ansfm_upload_dust) and the Rayleigh
// parametrisations: the one record of the arguments use_cia, lay_q, lay_frac, lay_totam, lay_delh, use_dust, lay_cont, ray_mode
// and f4 of include/ansfm.h, with the layer temperatures the CIA reads.  RtCall and MsCall carry it with the caller's
// pointers, a staged copy and the launchers with device pointers over the n * L layers of the call; an array whose term is
// off is null.  (An entry that checks the arguments further down brace-initialises it: the order of the fields stays.)
struct ContCall {
    int ISPACE = 0, use_cia = 0, use_dust = 0, ray_mode = 0;
    const double *temp = nullptr, *q = nullptr, *frac = nullptr, *totam = nullptr, *delh = nullptr, *cont = nullptr, *f4 = nullptr;
};
// ansfm_ops.hip: what every entry with a fused continuum refuses about those arguments, ANSFM_ERR_INVALID each -- a ray_mode
// other than IRAY 0, 1, 2, 4 or 12 (calc_tau_rayleighv), mode 4 without f4, a term without its arrays, a term that `need`
// asks for and the call leaves off, CIA without a resident source or with one of the other ISPACE, aerosols without a
// resident source -- and the record of a call that passes.  fn: the entry's name and ": ".
enum class ContNeed {
    any_term,    // thermal forward and gradient, ansfm_cirsrad_ck_scatter_batch_cont: something must form a continuum
    scatterer,   // single scattering: aerosols or Rayleigh scattering, or nothing scatters
    aerosols     // ansfm_cirsrad_ck_scatter_batch_src: the phase functions are those of the aerosol populations
};
int fused_cont_check(ansfm_ctx *ctx, const std::string &fn, int ISPACE, const double *lay_temp, int use_cia, const double *lay_q,
                     const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust, const double *lay_cont,
                     int ray_mode, const double *f4, ContNeed need, ContCall *out);
// the record of model m of a batch of L layers each
inline ContCall cont_of_model(const ansfm_ctx *ctx, ContCall c, size_t m, int L)
{
    const auto at = [&](const double *&a, size_t width) { if (a) a += m * L * width; };
    at(c.temp, 1); at(c.q, ctx->cia_NVMR); at(c.frac, 1); at(c.totam, 1); at(c.delh, 1); at(c.cont, ctx->dust_n); at(c.f4, 4);
    return c;
}
// ansfm_api.hip: dedup_rows with the columns the continuum of c is formed from as part of a layer's identity -- the column
// (CIA, Rayleigh), the Rayleigh composition (ray_mode 4), the mixing ratios and the thickness (CIA), the para-H2 fraction and
// the aerosol columns.  frac_always: the para-H2 fraction counts whenever CIA is on (the thermal route); otherwise only where
// cia_layer reads it, a table with a para-H2 axis (the scattering routes)
int dedup_rows_cont(ansfm_ctx *ctx, int n, int L, const double *press, const double *temp, const double *amount, const ContCall &c,
                    bool frac_always, DedupRows *out);
// ansfm_api.hip, what the gradient RT entries and the transit entry (ansfm_transit.hip) share (described where they are
// defined): the gas stage of a gradient call, the merge slot behind every parameter, the end of a call without a generic rerun
int grad_gas_stage(ansfm_ctx *ctx, int n_models, int L, const double *lay_press_pa, const double *lay_temp, const double *amount,
                   const double *taucont, const double *dtaucon, int NPAR, const double **cont_t, const double **dcont_t,
                   const ContCall *fused = nullptr, int NVMR = 0);
int fill_slot_of_param(ansfm_ctx *ctx, const int32_t *igas_map_host, int NVMR, int NPAR, unsigned gas_mask,
                       signed char *slot_of_param);
int check_unsorted(ansfm_ctx *ctx);
// ansfm_lbl.hip: k_lblrt_tau for gas_tau, on the n models from m0 of the state of ansfm_lblrt_set_state
void launch_lblrt_tau(ansfm_ctx *ctx, int n, int L, int m0, const double *amount, double *dk);
// ansfm_ops.hip: k_tau_rayleigh_rows for the thermal branch, into ctx->cont_t [rows][Wpad]; slot_rows: the de-duplication's work
// list, or nullptr for every (model, layer) in order
void launch_tau_rayleigh_rows(ansfm_ctx *ctx, int rows, int ray_mode, int ISPACE, const int32_t *slot_rows, const double *ray_totam,
                              const double *ray_f4);
// ansfm_ops.hip: k_cia_rows_prep + k_tau_cont_rows for the thermal branch, into ctx->cont_t [rows][Wpad]: (TAUCIA + TAUDUST) +
// TAURAY of the rows from the resident sources (ContCall, above)
int launch_tau_cont_rows(ansfm_ctx *ctx, int rows, const int32_t *slot_rows, const ContCall &c);
// ansfm_ops.hip: k_cia_rows_prep + k_ms_cont_rows for the multiple-scattering batch, into ctx->ms_cont_rows: the five arrays of
// the rows in the layout ansfm_cirsrad_ck_scatter_batch_rows takes, [rows][W] / [rows][NDUST][W]; a term that is not used is null
struct MsContRows { const double *cia, *dust, *ray, *sca, *lf; };
int launch_ms_cont_rows(ansfm_ctx *ctx, int rows, const int32_t *slot_rows, const ContCall &c, MsContRows *out);
// ansfm_ops.hip: k_cia_rows_prep + k_ss_cont_rows for the single-scattering batch: the continuum into ctx->cont_t [rows][Wpad], the
// scattering opacity [rows][Wpad] and the layer-mean phase function of the P paths [P][rows][Wpad] into ctx->ss_cont_rows;
// phase_fn [W][P][NDUST + 1] on the device
struct SsContRows { const double *cont, *sca, *phase; };
int launch_ss_cont_rows(ansfm_ctx *ctx, int rows, const int32_t *slot_rows, const ContCall &c, int P, const double *phase_fn,
                        SsContRows *out);
// ansfm_ops.hip: k_dtau_cont_rows for the gradient thermal branch, into ctx->dcont_t [n][NPAR][L][Wpad]: dTAUCON of the n * L
// layers from the resident sources.  After launch_tau_cont_rows(ctx, n * L, nullptr, c) on the same stream: the CIA records in
// ctx->cia_lay are that launch's.
int launch_dtau_cont_rows(ansfm_ctx *ctx, int n_models, int L, int NVMR, int NPAR, const ContCall &c);

// ansfm_phase.hip, for the fused scattering entries.  phase_source_check: ANSFM_ERR_INVALID unless a phase-function source of
// ncont populations stands; phase_source_angles: the host's checks of the angles of a launch (IMIE 1: inside Scatter.THETA).
// launch_phase_source: k_phase_fn on the source at theta_deg [nth] (host), on ctx->stream, into out on the device --
// mu_theta = nullptr: [W][nth][NDUST + ray], ray != 0 with calc_phase_ray behind the populations (phase_fn of the
// single-scattering batch); mu_theta [nth] (host): phasarr [NDUST][W][2][nth] of the scattering entries
int phase_source_check(ansfm_ctx *ctx, const std::string &fn, int ncont);
int phase_source_angles(ansfm_ctx *ctx, const std::string &fn, int nth, const double *theta_deg);
int launch_phase_source(ansfm_ctx *ctx, int nth, const double *theta_deg, const double *mu_theta, int ray, double *out);

// ansfm_overlap.hip / ansfm_overlapg.hip: k_ck_overlap (or k_ck_overlap32) and k_ck_overlapg over n_models x L layers into tau
// (and dk); from_k: the array-level seams' k (and dkdT) instead of the table; generic: per-lane sort first (rerun of an unsorted call)
struct LayerInterp;
struct OverlapParams;
int launch_overlap(ansfm_ctx *ctx, bool from_k, const double *kin, int W, int Wpad, int G, int S, int L, int n_models,
                   const LayerInterp *li, const double *amount, const double *del_g_dev, const double *del_g_host, double *tau,
                   bool generic);
int launch_overlapg(ansfm_ctx *ctx, bool from_k, const double *kin, const double *dkin, int W, int Wpad, int G, int S, int L,
                    int n_models, const LayerInterp *li, const double *amount, const double *del_g_dev, const double *del_g_host,
                    double *tau, double *dk, bool generic);
// ansfm_overlap.hip: what the two 64-bit-key merge launches set up alike, in two calls because the forward launch plans its
// kernel, and with it the LDS size and the grid (ansfm_merge_plan.h), from g_ord.  merge_params: the fields of p both kernels read, the g_ord table (float32
// cumulative sum when DELG is float32, NaN after the last boundary) and the tile counter's address; p was zeroed by the caller.
void merge_params(ansfm_ctx *ctx, OverlapParams &p, const double *kin, int W, int Wpad, int G, int S, int L, int n_models,
                  const LayerInterp *li, const double *amount, const double *del_g_dev, const double *del_g_host, double *tau);
// merge_launch_begin: reserves grid x bytes_per_block of every workspace (grid: merge_grid or the plan's), then clears the
// tile counter on the stream.  The kernel launch follows.
struct MergeWorkspace {
    DevBuf *buf;
    size_t bytes_per_block;
};
int merge_launch_begin(ansfm_ctx *ctx, const OverlapParams &p, long grid, std::initializer_list<MergeWorkspace> workspaces);
// ansfm_rt.hip: k_thermal_rt by mode, batch size and prefix sharing; k_thermal_rtg with the largest reduction buffer that fits;
// the array-level gradient seam; dspec [P][NPAR][LIMAX][Wpad] -> dSPECOUT [W][NPAR][LIMAX][P] of one model
struct RtParams;
struct RtGParams;
int launch_rt(ansfm_ctx *ctx, const RtParams &p_in, int n_models);
int launch_rtg(ansfm_ctx *ctx, const RtGParams &q, int n_models);
void launch_thermal_emission_g_seam(ansfm_ctx *ctx, int ISPACE, int W, int G, int NPAR, int NLAYIN, int NVMR, const double *wave,
                                    const double *tau, const double *dtau, const double *temp, const double *press, double TSURF,
                                    const double *emis, double *o_spec, double *o_dspec, double *o_dts);
void launch_dspec_to_ref(ansfm_ctx *ctx, const double *src, double *dst, int W, int Wpad, int NPAR, int LIMAX, int P,
                         const int32_t *nlayin);

// What every CIRSrad entry point leaves behind after its last launch, for ansfm_last_kernel_ms, ansfm_get_taugas and
// ansfm_last_layer_rows: one merge and one RT launch between the events, of n_models x L layers
inline void call_recorded(ansfm_ctx *ctx, int n_models, int L)
{
    ctx->overlap_launches = 1;
    ctx->rt_launches = 1;
    ctx->overlap_ms = -1.0;  // resolved lazily in ansfm_last_kernel_ms
    ctx->last_n = n_models; ctx->last_L = L;
}

/* ---- host -> device staging of the host-pointer entry points --------------------------------------------------------- */
inline int h2d(ansfm_ctx *ctx, DevBuf &b, const void *src, size_t bytes, const void **out)
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

// The per-layer arrays of a fused continuum through the next six buffers of st, in this order: the record returned has the
// device copies of h's host arrays over nl = n * L layers and d_temp, the staged layer temperatures, in their place
inline ContCall stage_cont(Stager &st, ContCall h, size_t nl, const double *d_temp)
{
    const ansfm_ctx *ctx = st.ctx;
    h.temp = d_temp;
    h.q = st.up(h.q, nl * ctx->cia_NVMR); h.frac = st.up(h.frac, nl); h.totam = st.up(h.totam, nl);
    h.delh = st.up(h.delh, nl); h.cont = st.up(h.cont, nl * ctx->dust_n); h.f4 = st.up(h.f4, nl * 4);
    return h;
}

}  // namespace ansfm
